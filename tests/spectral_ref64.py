"""The yardstick for the spatial-frequency spectra (include/dt_hip_spectral.h), in plain numpy.

The same direct DFT as the header defines, F[u][v] = sum_y sum_x x[y][x] exp(-2 pi i (u y / H + v x / W)), with every
product and sum in ``np.longdouble`` (x87 extended: unit roundoff 2^-64, 2048 times below fp64's).  The twiddle factors
come from a long-double pi with the index reduced mod N first, so no angle above 2 pi is formed; all H x W coefficients
are transformed (no use of the symmetry of a real picture).  Then the five sums per bin.

``forward_bound`` is the a-priori tolerance for a device output, derived below from the number formats, never from what
the device returns:

  * a coefficient computed in fp64 as two chained sums of at most W and H terms, with rounded products and twiddle
    factors that are themselves rounded, is within  delta(x) = (H + W + 8) 2^-53 sum|x|  of the true one: each of the
    W + H additions and the few roundings per term (product, twiddle) lose at most 2^-53 of a partial sum, and no partial
    sum exceeds sum|x| in magnitude;
  * |F'|^2 - |F|^2 = 2 Re(conj(F) e) + |e|^2 with |e| <= delta, so a bin of m cells of P is within
    sum_cells (2 |F| delta + delta^2) + (m + 2) 2^-53 sum_cells P:  the second term is the m additions of the bin and the
    two roundings inside a cell's own |F|^2;
  * a cell of A conj(B) moves by at most |A| delta_b + |B| delta_a + delta_a delta_b, in its real and in its imaginary
    part; the additions are bounded with sum_cells |A||B|;
  * D is P of the picture a - b (exact in fp64), so its delta is delta(a - b): it shrinks with the difference, which is
    what an implementation that subtracts powers cannot meet.

tests/test_spectral_host.py checks that a plain sequential float64 transform stays below a tenth of delta.
"""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
U = 2.0 ** -53                     # unit roundoff of fp64
PI = LD("3.14159265358979323846264338327950288")
PA, PB, CRE, CIM, D = range(5)
NAMES = ("power_a", "power_b", "cross_re", "cross_im", "error")


def twiddles(N, dtype=CLD):
    """exp(-2 pi i k / N) for k = 0 .. N-1"""
    ang = -2 * PI * np.arange(N, dtype=LD) / LD(N)
    return (np.cos(ang) + 1j * np.sin(ang)).astype(dtype)


def dft_matrix(N, dtype=CLD):
    """M[u][y] = exp(-2 pi i ((u y) mod N) / N)"""
    k = np.arange(N)
    return twiddles(N, dtype)[(k[:, None] * k[None, :]) % N]


def dft2(x):
    """the unnormalised forward DFT over the last two axes of a real array, in extended precision"""
    x = np.asarray(x).astype(LD)
    H, W = x.shape[-2:]
    rows = x.astype(CLD) @ dft_matrix(W).T            # along x
    return dft_matrix(H) @ rows                       # along y


def dft2_plain64(x):
    """a plain float64 implementation: the terms of each of the two sums added one after the other"""
    x = np.asarray(x).astype(np.float64)
    H, W = x.shape[-2:]
    mw, mh = dft_matrix(W, np.complex128), dft_matrix(H, np.complex128)
    rows = np.zeros(x.shape[:-1] + (W,), dtype=np.complex128)
    for k in range(W):
        rows = rows + x[..., :, k, None] * mw[:, k]
    out = np.zeros_like(rows)
    for k in range(H):
        out = out + mh[:, k, None] * rows[..., k, None, :]
    return out


def delta(x):
    """the coefficient bound delta(x) of the module text, one number per picture (longdouble, shape x.shape[:-2])"""
    x = np.asarray(x).astype(LD)
    H, W = x.shape[-2:]
    return LD((H + W + 8) * U) * np.abs(x).sum(axis=(-2, -1))


def bin_sum(values, table, n_bins):
    """[..., H, W] -> [..., n_bins]: the cells of every bin added (cells with a table entry outside [0, n_bins) left out)"""
    values = np.asarray(values)
    table = np.asarray(table)
    lead = values.shape[:-2]
    flat = values.reshape((-1, table.size))
    keep = (table.ravel() >= 0) & (table.ravel() < n_bins)
    out = np.zeros((flat.shape[0], n_bins), dtype=values.dtype)
    for r in range(flat.shape[0]):
        np.add.at(out[r], table.ravel()[keep], flat[r][keep])
    return out.reshape(lead + (n_bins,))


def difference(a, b):
    """double(a) - double(b), which is exact"""
    return np.asarray(a, dtype=np.float32).astype(np.float64) - np.asarray(b, dtype=np.float32).astype(np.float64)


def spectra(a, b):
    """(A, B, Delta) of the header for pictures a, b [..., H, W] float32; Delta = DFT(double(a) - double(b))"""
    return dft2(np.asarray(a, dtype=np.float32)), dft2(np.asarray(b, dtype=np.float32)), dft2(difference(a, b))


def pair_sums(a, b, table, n_bins, made=None):
    """[..., n_bins, 5] longdouble for pictures a, b [..., H, W] float32: P_a, P_b, C_re, C_im, D of the header
    (``made``: ``spectra(a, b)`` where the caller has them already)"""
    A, B, Dl = spectra(a, b) if made is None else made
    cross = A * np.conj(B)
    cells = [np.abs(A) ** 2, np.abs(B) ** 2, cross.real, cross.imag, np.abs(Dl) ** 2]
    return np.stack([bin_sum(c.astype(LD), table, n_bins) for c in cells], axis=-1)


def power_sums(a, table, n_bins):
    """[..., n_bins] longdouble: P_a alone"""
    return bin_sum((np.abs(dft2(np.asarray(a, dtype=np.float32))) ** 2).astype(LD), table, n_bins)


def forward_bound(a, b, table, n_bins, made=None):
    """[..., n_bins, 5] longdouble: the tolerance of each output of ``pair_sums`` (module text)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    d = difference(a, b)
    mA, mB, mD = (np.abs(F).astype(LD) for F in (spectra(a, b) if made is None else made))
    da, db, dd = (delta(x)[..., None, None] for x in (a, b, d))
    table = np.asarray(table)
    m = np.bincount(table.ravel()[(table.ravel() >= 0) & (table.ravel() < n_bins)], minlength=n_bins).astype(LD)
    s = lambda cells: bin_sum(cells, table, n_bins)
    tail = (m + 2) * LD(U)
    power = lambda mag, dl: s(2 * mag * dl + dl * dl) + tail * s(mag * mag)
    cross = s(mA * db + mB * da + da * db) + tail * s(mA * mB)
    return np.stack([power(mA, da), power(mB, db), cross, cross, power(mD, dd)], axis=-1)


def status(a, b=None):
    """[...] int: 1 for a row [..., C, H, W] with a NaN or Inf in it (in either set)"""
    bad = ~np.isfinite(np.asarray(a)).all(axis=(-3, -2, -1))
    if b is not None:
        bad |= ~np.isfinite(np.asarray(b)).all(axis=(-3, -2, -1))
    return bad.astype(np.int32)


def pictures(seed, shape, kind):
    """The inputs of the tolerance checks, float32 (teacher, student) of ``shape`` [..., C, H, W]: ``gauss`` two independent
    standard normal sets; ``offset`` the same plus 100 (the DC term dominates every sum); ``near`` the student is the
    teacher plus 1e-3 of a standard normal"""
    rs = np.random.RandomState(seed)
    a, e = rs.standard_normal(shape), rs.standard_normal(shape)
    if kind == "gauss":
        return a.astype(np.float32), e.astype(np.float32)
    if kind == "offset":
        return (a + 100.0).astype(np.float32), (e + 100.0).astype(np.float32)
    if kind == "near":
        a = a.astype(np.float32)
        return a, (a + np.float32(1e-3) * e.astype(np.float32)).astype(np.float32)
    raise ValueError(kind)


def holes_table(H, W, n_bins=3):
    """a table that is not radial: bin (3 u + 5 v) mod n_bins, with -1 (left out) on every cell whose index is a multiple
    of 4 -- DC among them"""
    u, v = np.arange(H)[:, None], np.arange(W)[None, :]
    t = ((3 * u + 5 * v) % n_bins).astype(np.int32)
    t[(u * W + v) % 4 == 0] = -1
    return t, n_bins


def cell_table(H, W):
    """one bin per coefficient"""
    return np.arange(H * W, dtype=np.int32).reshape(H, W), H * W
