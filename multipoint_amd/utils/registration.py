"""Keypoint-free initial transform: Fourier-Mellin phase correlation on gradient magnitude (csrc/register.hip, csrc/fft.hip;
DESIGN.md 3.20).  A similarity (rotation, scale, two translations) optical -> thermal from the frames themselves, pooled over
the pairs of a group the way pool_matches pools matches: the normalised cross-power spectra of a group's pairs add.

Stages, every one a HIP kernel (PyTorch only holds the memory):
  register_prepare      Hann-windowed gradient magnitude of a frame, optionally read through a similarity about the frame centre,
                        centred in a zeroed N x N complex plane
  register_logpolar     log1p|F| of a spectrum on a log-polar grid over the half plane
  register_cross_power  sum over a group's pairs of a conj(b) / |a conj(b)|
  register_peak         maximum, its 3-point parabola offsets with wrapped neighbours, the signed position, the largest value
                        outside the wrapped 3 x 3 block around it

Conventions (derived in DESIGN.md 3.20): q = s R(theta) p + d maps an optical pixel p = (x, y) to the thermal pixel q, R(theta) =
[[cos, -sin], [sin, cos]] with y pointing down.  A correlation peak at position p of planes (a, b) means a(x) = b(x - p).  The
stage-1 peak is (-theta A / pi, ln(s) / step) in (angle, radius) bins."""
import collections
import math

import numpy as np
import torch

from .. import _lib

__all__ = ['RegistrationPeaks', 'FourierReport', 'fft_length_at_least', 'hann_table', 'logpolar_tables', 'register_prepare',
           'register_logpolar', 'register_cross_power', 'register_peak', 'phase_correlation', 'FourierEstimator',
           'estimate_similarity_fourier', 'compose_fourier_transform', 'DEFAULT_R_MIN_FRACTION']

RegistrationPeaks = collections.namedtuple('RegistrationPeaks', 'index offset signed peak second')
RegistrationPeaks.__doc__ = """register_peak's result for G planes: index [G,2] int32 (row, column) of the maximum (the first in
row-major order on a tie); offset [G,2] float32, the parabola offsets per axis; signed [G,2] float32, index folded to signed form
(an index above size / 2 becomes negative) plus offset; peak [G] float32; second [G] float32, the largest value outside the
wrapped 3 x 3 block around the maximum (-inf when the plane has no such value)."""

DEFAULT_R_MIN_FRACTION = 1.0 / 32.0      # r_min of the log-polar grid as a fraction of N


def fft_length_at_least(n):
    """The smallest line length 2^a 3^b 5^c in [8, 4096] that is >= n."""
    from ..models.classic_detectors import fft_length_ok
    m = max(int(n), 8)
    while m <= 4096:
        if fft_length_ok(m):
            return m
        m += 1
    raise ValueError('registration: no FFT length >= %d (the largest is 4096)' % n)


def hann_table(n):
    """Symmetric Hann window of n samples, 0.5 - 0.5 cos(2 pi i / (n - 1)), in double, rounded to float32 (n == 1: 1)."""
    if n < 1:
        raise ValueError('hann_table: n must be positive')
    if n == 1:
        return np.ones(1, np.float32)
    i = np.arange(n, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / (n - 1))).astype(np.float32)


def logpolar_tables(N, A, R, r_min=None):
    """(ca [A], sa [A], rho [R], wr [R], step) of the log-polar grid of an N x N spectrum: angles a pi / A (the half plane),
    radii geometric from r_min (default N / 32, at least 1) to N / 2 - 1, a Hann window over the radii; float32 from double.
    step = ln(rho[r + 1] / rho[r])."""
    if N < 8 or A < 3 or R < 3:
        raise ValueError('logpolar_tables: need N >= 8, A >= 3, R >= 3')
    r_max = float(N // 2 - 1)
    r_min = max(1.0, N * DEFAULT_R_MIN_FRACTION) if r_min is None else float(r_min)
    if not 0.0 < r_min < r_max:
        raise ValueError('logpolar_tables: need 0 < r_min < N / 2 - 1, got %g' % r_min)
    ang = np.arange(A, dtype=np.float64) * (np.pi / A)
    step = math.log(r_max / r_min) / (R - 1)
    rho = r_min * np.exp(np.arange(R, dtype=np.float64) * step)
    return (np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32), rho.astype(np.float32), hann_table(R), step)


def compose_fourier_transform(cs, peak_yx, optical_hw, thermal_hw, N):
    """The 3x3 float64 optical -> thermal matrix from the similarity pair cs = (s cos theta, s sin theta) the thermal frames
    were prepared under and the signed stage-2 peak (row, column) of (optical, prepared thermal): with A = [[c, -s], [s, c]],
    tau = off_o - off_t - peak and d = Ct - A (Ct - tau), Ct the thermal frame centre and off the windows' plane offsets."""
    (Ho, Wo), (Ht, Wt) = optical_hw, thermal_hw
    c, s = float(cs[0]), float(cs[1])
    A = np.array([[c, -s], [s, c]], np.float64)
    off_o = np.array([(N - Wo) // 2, (N - Ho) // 2], np.float64)
    off_t = np.array([(N - Wt) // 2, (N - Ht) // 2], np.float64)
    tau = off_o - off_t - np.array([float(peak_yx[1]), float(peak_yx[0])])
    ct = np.array([(Wt - 1) / 2.0, (Ht - 1) / 2.0])
    d = ct - A @ (ct - tau)
    T = np.eye(3)
    T[:2, :2] = A
    T[:2, 2] = d
    return T


# ----------------------------------------------------------------------------------------------------------------------
# the four kernels
# ----------------------------------------------------------------------------------------------------------------------
def _real_view(x, what):
    if x.dtype != torch.complex64 or x.dim() != 3:
        raise ValueError('%s: need a complex64 tensor [n, h, w], got %s %s' % (what, tuple(x.shape), x.dtype))
    return torch.view_as_real(x.contiguous())


def register_prepare(frames, N, cs=None):
    """frames float32 [n,H,W] -> complex64 [n,N,N] (mp_register_prepare).  cs: float32 [n,2] of (cos * scale, sin * scale), the
    similarity about the frame centre every tap is read through; None: the identity."""
    dev = _lib.require_cuda(frames.device)
    if frames.dim() != 3 or frames.dtype != torch.float32:
        raise ValueError('register_prepare: frames must be float32 [n, H, W]')
    n, H, W = frames.shape
    frames = frames.contiguous()
    if cs is not None:
        cs = torch.as_tensor(cs, dtype=torch.float32).to(dev).contiguous()
        if cs.shape != (n, 2):
            raise ValueError('register_prepare: cs must be [%d, 2]' % n)
    wy = torch.from_numpy(hann_table(H)).to(dev)
    wx = torch.from_numpy(hann_table(W)).to(dev)
    out = torch.empty((n, N, N, 2), dtype=torch.float32, device=dev)
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_register_prepare(h.ptr, _lib.ptr(frames), _lib.ptr(cs), _lib.ptr(wy), _lib.ptr(wx), n, H, W, int(N),
                                          _lib.ptr(out), _lib.stream_ptr(dev)))
    return torch.view_as_complex(out)


def register_logpolar(spectrum, A, R, r_min=None):
    """spectrum complex64 [n,N,N] (FFT order) -> complex64 [n,A,R] (mp_register_logpolar) on the grid of logpolar_tables."""
    dev = _lib.require_cuda(spectrum.device)
    sr = _real_view(spectrum, 'register_logpolar')
    n, N = spectrum.shape[0], spectrum.shape[1]
    if spectrum.shape[2] != N:
        raise ValueError('register_logpolar: the spectrum must be square')
    ca, sa, rho, wr, _ = logpolar_tables(N, A, R, r_min)
    tab = torch.from_numpy(np.concatenate([ca, sa, rho, wr])).to(dev)
    out = torch.empty((n, A, R, 2), dtype=torch.float32, device=dev)
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_register_logpolar(h.ptr, _lib.ptr(sr), n, N, _lib.ptr(tab), _lib.ptr(tab[A:]), _lib.ptr(tab[2 * A:]),
                                           _lib.ptr(tab[2 * A + R:]), int(A), int(R), _lib.ptr(out), _lib.stream_ptr(dev)))
    return torch.view_as_complex(out)


def register_cross_power(a, b, group_offsets=None, out=None):
    """Sum over the pairs of every group of a conj(b) / |a conj(b)| (mp_register_cross_power): a, b complex64 [P,h,w],
    group_offsets int32 [G+1] (None: one group of all pairs) -> complex64 [G,h,w].  With `out` (a former result) the sums
    continue from it in pair order: a batch fed in chunks gives the bits of one call."""
    dev = _lib.require_cuda(a.device)
    ar, br = _real_view(a, 'register_cross_power'), _real_view(b, 'register_cross_power')
    if a.shape != b.shape:
        raise ValueError('register_cross_power: a and b must have one shape')
    P, hh, ww = a.shape
    if group_offsets is None:
        group_offsets = torch.tensor([0, P], dtype=torch.int32)
    go = torch.as_tensor(group_offsets).to(device=dev, dtype=torch.int32).contiguous()
    goh = go.cpu().numpy()
    if go.dim() != 1 or len(goh) < 2 or goh[0] != 0 or goh[-1] != P or (np.diff(goh) < 0).any():
        raise ValueError('register_cross_power: group_offsets must be non-decreasing from 0 to %d' % P)
    G = len(goh) - 1
    if out is None:
        res = torch.empty((G, hh, ww, 2), dtype=torch.float32, device=dev)
    else:
        if out.dtype != torch.complex64 or out.shape != (G, hh, ww) or not out.is_contiguous():
            raise ValueError('register_cross_power: out must be a contiguous complex64 [%d, %d, %d]' % (G, hh, ww))
        res = torch.view_as_real(out)
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_register_cross_power(h.ptr, _lib.ptr(ar), _lib.ptr(br), _lib.ptr(go), P, G, hh, ww,
                                              0 if out is None else 1, _lib.ptr(res), _lib.stream_ptr(dev)))
    return torch.view_as_complex(res)


def register_peak(planes):
    """planes float32 [G,h,w], or complex64 [G,h,w] whose real part is searched -> RegistrationPeaks (mp_register_peak)."""
    dev = _lib.require_cuda(planes.device)
    if planes.dim() != 3 or planes.dtype not in (torch.float32, torch.complex64):
        raise ValueError('register_peak: need float32 or complex64 [G, h, w]')
    G, hh, ww = planes.shape
    stride = 2 if planes.dtype == torch.complex64 else 1
    data = torch.view_as_real(planes.contiguous()) if stride == 2 else planes.contiguous()
    import ctypes
    nbytes = ctypes.c_longlong()
    h = _lib.get_handle(dev)
    h.check(h.lib.mp_register_peak_workspace_bytes(G, hh, ww, ctypes.byref(nbytes)))
    ws = torch.empty((max(nbytes.value, 16),), dtype=torch.uint8, device=dev)
    oi = torch.empty((G, 2), dtype=torch.int32, device=dev)
    of = torch.empty((G, 6), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_register_peak(h.ptr, _lib.ptr(data), G, hh, ww, stride, _lib.ptr(oi), _lib.ptr(of), _lib.ptr(ws),
                                       ws.numel(), _lib.stream_ptr(dev)))
    return RegistrationPeaks(oi, of[:, 0:2], of[:, 2:4], of[:, 4], of[:, 5])


def _correlation_surface(x):
    """Unnormalised inverse FFT of pooled cross-power sums, scaled by 1 / (h w): a single perfect pair peaks at 1."""
    from ..models.classic_detectors import fft2d
    s = fft2d(x, inverse=True)
    return s * (1.0 / (x.shape[-2] * x.shape[-1]))


def phase_correlation(planes_a, planes_b, group_offsets=None):
    """Pooled phase correlation of complex64 planes [P,h,w] (h, w FFT lengths): RegistrationPeaks of the [G] surfaces
    ifft(sum_pairs A conj(B) / |A conj(B)|) / (h w).  A peak at signed position p means a(x) = b(x - p)."""
    from ..models.classic_detectors import fft2d
    x = register_cross_power(fft2d(planes_a), fft2d(planes_b), group_offsets)
    return register_peak(_correlation_surface(x))


# ----------------------------------------------------------------------------------------------------------------------
# the driver
# ----------------------------------------------------------------------------------------------------------------------
FourierReport = collections.namedtuple('FourierReport', 'angle scale dx dy peak1 second1 peak2 second2 branch')
FourierReport.__doc__ = """Per group (float64 / int arrays [G]): angle, scale, dx, dy of the optical -> thermal transform in the
convention of decompose_similarity; peak and second of stage 1 (angle, scale) and of stage 2 (translation); branch, 1 where the
theta + pi candidate won stage 2."""


class FourierEstimator:
    """The pooled estimate in two accumulating passes, for batches that come in chunks: add_stage1(optical, thermal, groups) for
    every chunk, finish_stage1(), add_stage2(optical, thermal, groups) for every chunk again, finish().  `groups`: the group id
    of every pair of the chunk (non-decreasing over the whole sequence of chunks), ids in [0, G)."""

    def __init__(self, optical_hw, thermal_hw, G=1, angles=None, radii=None, r_min=None):
        self.ohw, self.thw = tuple(int(v) for v in optical_hw), tuple(int(v) for v in thermal_hw)
        self.G = int(G)
        self.N = fft_length_at_least(max(self.ohw + self.thw))
        self.A = fft_length_at_least(self.N) if angles is None else int(angles)
        self.R = fft_length_at_least(self.N) if radii is None else int(radii)
        from ..models.classic_detectors import fft_length_ok
        if not (fft_length_ok(self.A) and fft_length_ok(self.R)):
            raise ValueError('estimate_similarity_fourier: angles and radii must be FFT lengths (2^a 3^b 5^c in [8, 4096])')
        self.r_min = r_min
        self.step = logpolar_tables(self.N, self.A, self.R, r_min)[4]
        self.x1 = None
        self.x2 = None
        self.cs = None
        self.surface1 = self.surface2 = None

    def _offsets(self, groups, P):
        g = np.zeros(P, np.int64) if groups is None else np.asarray(groups, np.int64)
        if g.shape != (P,) or (np.diff(g) < 0).any() or (P and (g.min() < 0 or g.max() >= self.G)):
            raise ValueError('FourierEstimator: groups must be %d non-decreasing ids in [0, %d)' % (P, self.G))
        return g, np.searchsorted(g, np.arange(self.G + 1), side='left').astype(np.int32)

    def _check(self, optical, thermal):
        if optical.dim() != 3 or thermal.dim() != 3 or optical.shape[0] != thermal.shape[0] or optical.shape[0] < 1:
            raise ValueError('estimate_similarity_fourier: optical [P,Ho,Wo] and thermal [P,Ht,Wt] of the same P >= 1')
        if tuple(optical.shape[1:]) != self.ohw or tuple(thermal.shape[1:]) != self.thw:
            raise ValueError('estimate_similarity_fourier: all optical frames must have one size, and all thermal frames one size')
        return optical.to(torch.float32), thermal.to(torch.float32)

    def add_stage1(self, optical, thermal, groups=None):
        from ..models.classic_detectors import fft2d
        optical, thermal = self._check(optical, thermal)
        _, go = self._offsets(groups, optical.shape[0])
        lo = register_logpolar(fft2d(register_prepare(optical, self.N)), self.A, self.R, self.r_min)
        lt = register_logpolar(fft2d(register_prepare(thermal, self.N)), self.A, self.R, self.r_min)
        self.x1 = register_cross_power(fft2d(lo), fft2d(lt), go, out=self.x1)

    def finish_stage1(self):
        if self.x1 is None:
            raise ValueError('FourierEstimator: no pairs were added')
        self.surface1 = _correlation_surface(self.x1)
        self.pk1 = register_peak(self.surface1)
        sg = self.pk1.signed.double().cpu().numpy()
        self.theta = -sg[:, 0] * (math.pi / self.A)
        self.scale = np.exp(sg[:, 1] * self.step)
        # the pair the kernel reads the thermal frames through, rounded once to float32; the transform is composed from the same
        self.cs = np.stack([self.scale * np.cos(self.theta), self.scale * np.sin(self.theta)], 1).astype(np.float32)
        return self.cs

    def add_stage2(self, optical, thermal, groups=None):
        from ..models.classic_detectors import fft2d
        optical, thermal = self._check(optical, thermal)
        g, go = self._offsets(groups, optical.shape[0])
        fo = fft2d(register_prepare(optical, self.N))
        cs = torch.from_numpy(self.cs[g]).to(optical.device)
        x = [register_cross_power(fo, fft2d(register_prepare(thermal, self.N, sign * cs)), go,
                                  out=None if self.x2 is None else self.x2[b])
             for b, sign in enumerate((1.0, -1.0))]
        if self.x2 is None:
            self.x2 = x

    def finish(self):
        if self.x2 is None:
            raise ValueError('FourierEstimator: no pairs were added to stage 2')
        self.surface2 = [_correlation_surface(x) for x in self.x2]
        pk = [register_peak(s) for s in self.surface2]
        peaks = np.stack([p.peak.double().cpu().numpy() for p in pk])
        branch = (peaks[1] > peaks[0]).astype(np.int64)
        self.pk2 = pk
        T = np.zeros((self.G, 3, 3))
        rep = {k: np.zeros(self.G) for k in FourierReport._fields}
        from .evaluation import decompose_similarity
        p1, s1 = self.pk1.peak.double().cpu().numpy(), self.pk1.second.double().cpu().numpy()
        for g in range(self.G):
            b = int(branch[g])
            sg = pk[b].signed[g].double().cpu().numpy()
            T[g] = compose_fourier_transform((1.0, -1.0)[b] * self.cs[g].astype(np.float64), sg, self.ohw, self.thw, self.N)
            rep['angle'][g], rep['scale'][g], rep['dx'][g], rep['dy'][g] = decompose_similarity(T[g])
            rep['peak1'][g], rep['second1'][g] = p1[g], s1[g]
            rep['peak2'][g], rep['second2'][g] = float(pk[b].peak[g]), float(pk[b].second[g])
        rep['branch'] = branch
        return T, FourierReport(**rep)


def estimate_similarity_fourier(optical, thermal, groups=None, angles=None, radii=None, r_min=None):
    """One optical -> thermal similarity per group of pairs from Fourier-Mellin phase correlation.  optical float32 [P,Ho,Wo],
    thermal float32 [P,Ht,Wt] on the GPU, values in [0, 1] (the two sizes may differ); groups: None for one model per pair, or
    the non-decreasing group id of every pair as for pool_matches.  The planes are N x N, N the smallest FFT length >= the
    largest side; angles, radii: the log-polar grid, default the smallest FFT length >= N.
    Returns (transforms float64 [G,3,3], FourierReport)."""
    P = optical.shape[0]
    if groups is None:
        gid = np.arange(P)
    else:
        from .evaluation import _group_ids
        gid, _ = _group_ids(groups, P)
        if gid is None:
            gid = np.zeros(P, np.int64)
    G = int(gid.max()) + 1
    est = FourierEstimator(optical.shape[1:], thermal.shape[1:], G, angles, radii, r_min)
    est.add_stage1(optical, thermal, gid)
    est.finish_stage1()
    est.add_stage2(optical, thermal, gid)
    return est.finish()
