"""CPU: what the result views promise without a GPU -- the C ABI's plumbing, the palette, the new flags of the
command lines, properties of the numpy restatement the kernels are held to (tests/drawing_restatement.py), and the second
phase of check_alignment.py, which only moves files."""
import os
import re

import numpy as np
import pytest
import torch

import drawing_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('mp_draw_gray_to_rgb', 'mp_draw_marks', 'mp_draw_matches', 'mp_draw_compose')


def test_plumbing():
    from multipoint_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'multipoint_hip.h')).read()
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ENTRIES:
        m = re.search(r'\bint %s\(([^;]*)\);' % name, header)
        assert m, '%s is not declared in the header' % name
        params = [p for p in m.group(1).replace('\n', ' ').split(',') if p.strip()]
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(params), name
        assert params[0].strip() == 'mp_handle* h' and params[-1].strip() == 'void* stream'        # every entry takes a stream
        assert '`%s`' % name in integration, '%s is missing from INTEGRATION.md' % name
    assert sorted(n for n in _lib.SIGNATURES if n.startswith('mp_draw_')) == sorted(ENTRIES)
    assert 'draw.hip' in build.SOURCES and build.SCRATCH_CAPS['draw.hip'] == 0
    assert os.path.exists(os.path.join(build.CSRC, 'draw.hip'))
    assert '#define MP_DRAW_MAX_RADIUS 64' in header and _lib.MP_DRAW_MAX_RADIUS == 64 == R.MAX_RADIUS
    for table, names in ((_lib.MP_DRAW_KINDS, R.KINDS), (_lib.MP_DRAW_MODES, R.MODES)):
        assert tuple(table) == names
        for name, value in table.items():
            assert re.search(r'#define MP_DRAW_%s %d\b' % (name.upper(), value), header)
    import multipoint_amd.utils as U
    from multipoint_amd.utils import drawing
    for name in drawing.__all__:
        assert getattr(U, name) is getattr(drawing, name)


def test_match_palette():
    import colorsys
    from multipoint_amd.utils import drawing
    p = drawing.match_palette()
    assert p.dtype == np.uint8 and p.shape == (64, 3) and np.array_equal(p, drawing.match_palette(64))
    assert len({tuple(c) for c in p}) == 64
    assert np.array_equal(drawing.match_palette(5), p[:5])
    for i in (0, 1, 17, 63):
        want = [round(255 * c) for c in colorsys.hsv_to_rgb((i * 0.618033988749895) % 1.0, 1.0, 1.0)]
        assert p[i].tolist() == want
    assert p[0].tolist() == [255, 0, 0] and (p.max(1) == 255).all() and (p.min(1) == 0).all()      # fully saturated hues


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        return
    from multipoint_amd.utils import drawing
    with pytest.raises(RuntimeError):
        drawing.gray_to_rgb(torch.zeros(4, 4))
    with pytest.raises(RuntimeError):
        drawing.draw_keypoints(torch.zeros((4, 4, 3), dtype=torch.uint8), np.zeros((1, 2), np.int64))
    with pytest.raises(RuntimeError):
        drawing.draw_matches(torch.zeros(4, 4), torch.zeros(4, 4), np.zeros((1, 2)), np.zeros((1, 2)), np.zeros(1))
    with pytest.raises(RuntimeError):
        drawing.compose(torch.zeros(4, 4), torch.zeros(4, 4), 'blend')


def test_new_flags_parse_and_are_marked_as_extensions():
    import align_images
    import check_alignment
    import predict_align_image_pair
    import predict_keypoints
    import show_image_pair_sample
    import show_keypoints
    a = predict_keypoints.build_parser().parse_args(['-p', '--plot-dir', 'out', '-r', '3', '-mask'])
    assert (a.plot, a.plot_dir, a.radius, a.mask) == (True, 'out', 3, True)
    assert predict_keypoints.build_parser().parse_args([]).plot_dir is None
    a = predict_align_image_pair.build_parser().parse_args(['-p', '--plot-dir', 'out'])
    assert (a.plot, a.plot_dir) == (True, 'out') and predict_align_image_pair.build_parser().parse_args([]).plot_dir is None
    a = align_images.build_parser().parse_args(['--save-candidates'])
    assert a.save_candidates and not align_images.build_parser().parse_args([]).save_candidates
    a = show_keypoints.build_parser().parse_args(['-d', 'd.npz', '-k', 'k.npz', '-n', '2', '-r', '5', '-o', 'out'])
    assert (a.dataset_file, a.keypoint_file, a.sample_number, a.radius, a.output_dir) == ('d.npz', 'k.npz', 2, 5, 'out')
    a = show_image_pair_sample.build_parser().parse_args(['-i', 'd.npz', '-k', 'k.npz', '-n', '1', '-r', '2', '-o', 'out'])
    assert (a.input_file, a.keypoint_file, a.sample_number, a.radius, a.output_dir) == ('d.npz', 'k.npz', 1, 2, 'out')
    assert show_image_pair_sample.build_parser().parse_args([]).keypoint_file is None
    a = check_alignment.build_parser().parse_args(['-i', 'dir', '-dt', '250', '--review-dir', 'r', '--decisions', 'f'])
    assert (a.input_dir, a.dt, a.review_dir, a.decisions) == ('dir', 250, 'r', 'f')
    assert check_alignment.build_parser().parse_args([]).dt == 500
    for module, flags in ((predict_keypoints, ['--plot-dir']), (predict_align_image_pair, ['--plot-dir']),
                          (align_images, ['--save-candidates']), (show_keypoints, ['--output-dir']),
                          (show_image_pair_sample, ['--output-dir']), (check_alignment, ['--review-dir', '--decisions'])):
        text = ' '.join(module.build_parser().format_help().split())
        for flag in flags:
            assert re.search(re.escape(flag) + r'( [A-Z_]+)? \(extension', text), (module.__name__, flag)


@pytest.mark.parametrize('r', [0, 1, 2, 4, 6, 17, 59, 64])
def test_restated_marks(r):
    c = (7, -3)
    d = R.disc(c, r)
    assert (c[0], c[1]) in d and len(R.disc(c, -1)) == 0
    # four-fold symmetry about the centre, and the transpose
    assert d == {(2 * c[0] - x, y) for x, y in d} == {(x, 2 * c[1] - y) for x, y in d}
    assert d == {(c[0] + (y - c[1]), c[1] + (x - c[0])) for x, y in d}
    # the disc reaches exactly r along the axes and is convex per row
    assert max(x for x, y in d) == c[0] + r and max(y for x, y in d) == c[1] + r
    for t in (1, 2, 3, 5):
        outer, inner = r + t // 2, r - (t + 1) // 2
        ring = R.ring(c, r, t)
        assert ring | R.disc(c, inner) == R.disc(c, outer) and not (ring & R.disc(c, inner))
        assert ring == {(2 * c[0] - x, y) for x, y in ring} == {(x, 2 * c[1] - y) for x, y in ring}
        assert ((c[0] + outer, c[1]) in ring) and (inner < 0) == (c in ring)
    cross = R.cross(c, r)
    assert len(cross) == 4 * r + 1 and cross <= d
    assert R.disc(c, 0) == {c} and sorted(R.ring((0, 0), 1, 1)) == [(-1, 0), (0, -1), (0, 1), (1, 0)]


def test_restated_segments():
    rng = np.random.default_rng(0)
    W, H = 80, 24
    ends = [((0, 0), (79, 23)), ((79, 0), (0, 23)), ((5, 5), (5, 5)), ((3, 7), (60, 7)), ((9, 2), (9, 20)), ((70, 3), (10, 9))]
    ends += [((int(rng.integers(W)), int(rng.integers(H))), (int(rng.integers(W)), int(rng.integers(H)))) for _ in range(40)]
    for a, b in ends:
        px = R.line_pixels(W, H, a, b)
        assert a in px and b in px and len(px) == len(set(px)) == max(abs(a[0] - b[0]), abs(a[1] - b[1])) + 1
        assert all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) == 1 for p, q in zip(px, px[1:]))        # 8-connected
    # a segment that misses the canvas, and one that is clipped to it
    assert R.line_pixels(W, H, (-5, -5), (-1, 30)) == []
    px = R.line_pixels(W, H, (-10, 5), (100, 5))
    assert px == [(x, 5) for x in range(W)]


def test_restated_conversion_and_views():
    x = np.array([-1.0, -0.0, 0.0, 0.5, 1.0, 2.0, np.nan, 1 / 255, 254.999 / 255], np.float32)
    assert R.to_u8(x).tolist() == [0, 0, 0, 127, 255, 255, 0, 1, 254]
    img = np.random.default_rng(1).random((1, 6, 7), dtype=np.float32) * 1.2 - 0.1
    assert np.array_equal(R.gray_values(img), (np.clip(img, 0, 1) * 255.0).astype(np.uint8))
    a = np.array([[[0.2, -1.0, 1.0, 0.6]]], np.float32)
    t = np.array([[[0.4, 0.4, 0.0, 0.6]]], np.float32)
    A, T = R.to_u8(np.maximum(a, 0))[0, 0].astype(int), R.to_u8(t)[0, 0].astype(int)
    assert R.compose(a, t, 'blend', 256)[0, 0, :, 0].tolist() == [A[0], T[1], A[2], A[3]]
    assert R.compose(a, t, 'blend', 0)[0, 0, :, 0].tolist() == T.tolist()
    assert R.compose(a, t, 'blend', 128)[0, 0, :, 1].tolist() == [(A[0] + T[0] + 1) >> 1, T[1], (A[2] + T[2] + 1) >> 1, A[3]]
    assert R.compose(a, t, 'checker', cell=1)[0, 0, :, 2].tolist() == [A[0], T[1], A[2], T[3]]
    assert R.compose(a, t, 'checker', cell=2)[0, 0, :, 2].tolist() == [A[0], T[1], T[2], T[3]]
    assert R.compose(a, t, 'anaglyph')[0, 0].tolist() == [[A[0], T[0], T[0]], [0, T[1], T[1]], [A[2], T[2], T[2]], [A[3], T[3], T[3]]]
    assert R.compose(a, t, 'difference')[0, 0, :, 0].tolist() == [abs(A[0] - T[0]), T[1], 255, 0]
    # the highest index wins, whatever the palette length
    canvas = R.draw_marks(np.zeros((1, 9, 9, 3), np.uint8), [[(4, 4), (4, 5), (4, 4)]], (3,), 2, 1, 'disc', [(1, 1, 1), (2, 2, 2)])
    assert canvas[0, 4, 4, 0] == 1 and canvas[0, 4, 7, 0] == 2 and canvas[0, 4, 2, 0] == 1 and canvas[0, 0, 0, 0] == 0


def _png(path, value):
    from PIL import Image
    Image.fromarray(np.full((4, 6), value, np.uint8)).save(str(path))


def test_check_alignment_decisions(tmp_path, capsys):
    import check_alignment
    best, every = tmp_path / 'aligned' / 'best', tmp_path / 'aligned' / 'all'
    best.mkdir(parents=True)
    every.mkdir()
    for k, index in enumerate(('000', '001', '002', '003', '004')):
        _png(best / (index + '_optical.png'), 10 + k)
        _png(best / (index + '_thermal.png'), 100 + k)
    _png(best / '001_thermal_raw.png', 201)
    _png(every / '002_optical_0.png', 50)
    _png(every / '002_optical_1.png', 51)
    (tmp_path / 'checked.log').write_text('004_optical.png\n')
    assert check_alignment.pending_pairs(str(tmp_path)) == ['%03d_optical.png' % i for i in range(4)]
    assert sorted(check_alignment.alternatives(str(tmp_path), '002')) == [0, 1]
    decisions = tmp_path / 'decisions.txt'
    decisions.write_text('# reviewed by hand\n000 r\n001 a\n\n002 1\n003 ?\n')
    assert check_alignment.read_decisions(str(decisions)) == [('000', 'r'), ('001', 'a'), ('002', 1), ('003', '?')]
    assert check_alignment.main(['-i', str(tmp_path), '--decisions', str(decisions)]) == 0
    assert 'Accepted 2 images out of 4' in capsys.readouterr().out
    accepted = tmp_path / 'aligned' / 'accepted'
    assert sorted(os.listdir(str(accepted))) == ['001_optical.png', '001_thermal.png', '001_thermal_raw.png', '002_optical.png',
                                                 '002_thermal.png']
    assert (accepted / '001_optical.png').read_bytes() == (best / '001_optical.png').read_bytes()
    assert (accepted / '001_thermal_raw.png').read_bytes() == (best / '001_thermal_raw.png').read_bytes()
    assert (accepted / '002_optical.png').read_bytes() == (every / '002_optical_1.png').read_bytes()
    assert (accepted / '002_thermal.png').read_bytes() == (best / '002_thermal.png').read_bytes()
    assert (tmp_path / 'checked.log').read_text() == '004_optical.png\n000_optical.png\n001_optical.png\n002_optical.png\n'
    assert check_alignment.pending_pairs(str(tmp_path)) == ['003_optical.png']
    # 'n' rejects like 'r'; a decided pair, an unknown token and a missing alternative are refused
    decisions.write_text('003 n\n')
    check_alignment.main(['-i', str(tmp_path), '--decisions', str(decisions)])
    assert 'Accepted 0 images out of 1' in capsys.readouterr().out and check_alignment.pending_pairs(str(tmp_path)) == []
    for text in ('003 a\n', '003 x\n', '003\n'):
        decisions.write_text(text)
        with pytest.raises(ValueError):
            check_alignment.main(['-i', str(tmp_path), '--decisions', str(decisions)])
    (tmp_path / 'checked.log').write_text('')
    decisions.write_text('000 7\n')
    with pytest.raises(ValueError):
        check_alignment.main(['-i', str(tmp_path), '--decisions', str(decisions)])
