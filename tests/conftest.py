import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line('markers', 'gpu: needs an MI355X (run with -m gpu on the GPU box)')


@pytest.fixture(scope='session', autouse=True)
def _oracle_c_lib():
    """The oracle's C restatement is test infrastructure: (re)build it once per session."""
    import __graft_entry__ as g
    g.build_oracle()


@pytest.fixture(scope='session')
def oracle():
    from oracle import mp_oracle
    return mp_oracle


@pytest.fixture(scope='session')
def golden_dir():
    return os.path.join(ROOT, 'tests', 'golden')
