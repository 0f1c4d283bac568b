"""A numpy restatement, in float32, of the torch CPU generator's ``randn`` stream: the yardstick of the device RNG.

What it restates (checked bit for bit against recorded and live ``torch.randn`` in tests/test_rng_host.py):

* ``manual_seed(s)`` seeds an mt19937 by ``init_genrand(s mod 2**32)``; every word is tempered as usual.
* ``torch.rand`` turns one word into a float: ``(w & 0xFFFFFF) * 2**-24``.
* A contiguous fp32 ``randn`` of ``E >= 16`` elements takes ``E`` words as uniforms ``u[0..E)`` and transforms every full group
  of 16 by Box-Muller: ``u1 = 1 - u[j]``, ``u2 = u[j + 8]``, ``r = sqrt(-2 log u1)``, ``theta = 2 pi u2``, ``out[j] = r cos theta``,
  ``out[j + 8] = r sin theta`` (j = 0..7 of the group).  If ``E % 16 != 0`` it takes 16 more words and recomputes the last 16
  outputs ``out[E - 16 .. E)`` from those.  So a draw costs ``words(E)`` = ``E`` or ``E + 16`` words.
* ``log`` and ``sincos`` are the cephes polynomials of ATen/native/cpu/avx_mathfun.h with the multiply-adds fused the way the
  compiled library fuses them (``fma`` below marks each fused pair; everything else is a single rounded fp32 operation).
* ``torch.get_rng_state()`` is 5056 bytes: seed (8), left (int32), seeded (4), next (8), 624 state words as uint64, then the
  normal-sample cache, which these paths leave alone.

``fma(a, b, c)`` is emulated as ``float32(float64(a) * float64(b) + float64(c))``: the product of two fp32 values is exact in
fp64.  ``E < 16`` is a different (double precision, scalar) path in torch and is not restated.
"""
import numpy as np

N, M = 624, 397
STATE_BYTES = 5056
_F = np.float32


def init_genrand(seed):
    """The 624-word key after ``manual_seed(seed)``; the first output needs a regeneration (position 624)."""
    s = np.empty(N, np.uint32)
    x = int(seed) & 0xFFFFFFFF
    s[0] = x
    for i in range(1, N):
        x = (1812433253 * (x ^ (x >> 30)) + i) & 0xFFFFFFFF
        s[i] = x
    return s


def regenerate(state):
    """The next block of 624 untempered words.  Word i needs old i, i + 1 and i + 397 mod 624, so three spans of 227, 227 and
    170 words each read only old values or values of an earlier span."""
    s = np.array(state, dtype=np.uint32)
    for lo, hi in ((0, 227), (227, 454), (454, 624)):
        i = np.arange(lo, hi)
        y = (s[i] & np.uint32(0x80000000)) | (s[(i + 1) % N] & np.uint32(0x7FFFFFFF))
        s[i] = s[(i + M) % N] ^ (y >> np.uint32(1)) ^ np.where(y & np.uint32(1), np.uint32(0x9908B0DF), np.uint32(0))
    return s


def temper(y):
    y = np.array(y, dtype=np.uint32)
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9D2C5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    y ^= y >> np.uint32(18)
    return y


class Stream:
    """An mt19937 walk: ``state`` (624 untempered words) and ``pos`` in 0..624, the index of the next word in it (624: the
    block is used up, or is a fresh key)."""

    def __init__(self, state_or_seed, pos=None):
        if np.ndim(state_or_seed) == 0:
            self.state, self.pos = init_genrand(state_or_seed), N
        else:
            self.state, self.pos = np.array(state_or_seed, dtype=np.uint32), int(N if pos is None else pos)
            assert self.state.shape == (N,) and 0 <= self.pos <= N

    def copy(self):
        return Stream(self.state, self.pos)

    def words(self, n):
        """The next ``n`` tempered words."""
        out = np.empty(n, np.uint32)
        k = 0
        while k < n:
            if self.pos == N:
                self.state, self.pos = regenerate(self.state), 0
            take = min(N - self.pos, n - k)
            out[k:k + take] = temper(self.state[self.pos:self.pos + take])
            self.pos += take
            k += take
        return out

    def skip(self, n):
        while n > 0:
            if self.pos == N:
                self.state, self.pos = regenerate(self.state), 0
            take = min(N - self.pos, n)
            self.pos += take
            n -= take


def mt19937_words(state_or_seed, n, skip=0, pos=None):
    """``n`` tempered words after skipping ``skip``, and the stream where it ends."""
    st = state_or_seed.copy() if isinstance(state_or_seed, Stream) else Stream(state_or_seed, pos)
    st.skip(skip)
    return st.words(n), st


def words(E):
    """Words one fp32 ``randn`` of ``E >= 16`` elements consumes."""
    if E < 16:
        raise ValueError("randn of fewer than 16 elements takes another path in torch")
    return E if E % 16 == 0 else E + 16


def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(_F)


_LOG_P = [_F(v) for v in (7.0376836292E-2, -1.1514610310E-1, 1.1676998740E-1, -1.2420140846E-1, 1.4249322787E-1,
                          -1.6668057665E-1, 2.0000714765E-1, -2.4999993993E-1, 3.3333331174E-1)]
_LOG_Q1, _LOG_Q2, _SQRTHF = _F(-2.12194440e-4), _F(0.693359375), _F(0.707106781186547524)
_DP = [_F(-0.78515625), _F(-2.4187564849853515625e-4), _F(-3.77489497744594108e-8)]
_SIN_P = [_F(-1.9515295891E-4), _F(8.3321608736E-3), _F(-1.6666654611E-1)]
_COS_P = [_F(2.443315711809948E-005), _F(-1.388731625493765E-003), _F(4.166664568298827E-002)]
_FOPI, _TWO_PI = _F(1.27323954473516), _F(2.0 * np.pi)
_HALF, _ONE = _F(0.5), _F(1.0)


def log_f32(x):
    """log256_ps for x > 0 (fp32 array) with the pinned fusion."""
    x = np.maximum(x.astype(_F), np.uint32(0x00800000).view(_F))
    bits = x.view(np.uint32)
    e = ((bits >> np.uint32(23)).astype(np.int32) - 0x7F).astype(_F) + _ONE
    x = ((bits & np.uint32(0x807FFFFF)) | _HALF.view(np.uint32)).view(_F)
    small = x < _SQRTHF
    tmp = np.where(small, x, _F(0))
    x = (x - _ONE).astype(_F)
    e = (e - np.where(small, _ONE, _F(0))).astype(_F)
    x = (x + tmp).astype(_F)
    z = (x * x).astype(_F)
    y = np.full_like(x, _LOG_P[0])
    for p in _LOG_P[1:]:
        y = fma(y, x, np.full_like(x, p))
    y = (y * x).astype(_F)
    y = fma(y, z, (e * _LOG_Q1).astype(_F))
    y = (y - (z * _HALF).astype(_F)).astype(_F)
    x = (x + y).astype(_F)
    return fma(e, np.full_like(x, _LOG_Q2), x)


def sincos_f32(x):
    """sincos256_ps (fp32 array) with the pinned fusion: returns (sin, cos)."""
    x = x.astype(_F)
    sign_sin = x.view(np.uint32) & np.uint32(0x80000000)
    x = np.abs(x)
    y = (x * _FOPI).astype(_F)
    j = y.astype(np.int32)                       # truncation
    j = (j + 1) & ~np.int32(1)
    y = j.astype(_F)
    sign_sin = sign_sin ^ ((j & 4).astype(np.uint32) << np.uint32(29))
    poly = (j & 2) == 0
    sign_cos = ((~(j - 2)) & 4).astype(np.uint32) << np.uint32(29)
    for dp in _DP:
        x = fma(y, np.full_like(x, dp), x)
    z = (x * x).astype(_F)
    c = np.full_like(x, _COS_P[0])
    c = fma(c, z, np.full_like(x, _COS_P[1]))
    c = fma(c, z, np.full_like(x, _COS_P[2]))
    c = (c * z).astype(_F)
    c = fma(c, z, -(z * _HALF).astype(_F))
    c = (c + _ONE).astype(_F)
    s = np.full_like(x, _SIN_P[0])
    s = fma(s, z, np.full_like(x, _SIN_P[1]))
    s = fma(s, z, np.full_like(x, _SIN_P[2]))
    s = (s * z).astype(_F)
    s = fma(s, x, x)
    zero = np.zeros_like(x)
    ysin2, ysin1 = np.where(poly, s, zero), np.where(poly, zero, c)
    s2, c2 = (s - ysin2).astype(_F), (c - ysin1).astype(_F)
    sin = (ysin1 + ysin2).astype(_F)
    cos = (c2 + s2).astype(_F)
    return (sin.view(np.uint32) ^ sign_sin).view(_F), (cos.view(np.uint32) ^ sign_cos).view(_F)


def uniform(w):
    return ((np.asarray(w, np.uint32) & np.uint32(0xFFFFFF)).astype(_F) * _F(2.0 ** -24)).astype(_F)


def transform16(w):
    """Box-Muller over groups of 16 words: ``w`` uint32 [..., 16] -> fp32 [..., 16]."""
    with np.errstate(all="ignore"):
        u = uniform(w)
        u1 = (_ONE - u[..., :8]).astype(_F)
        u2 = u[..., 8:]
        r = np.sqrt((_F(-2.0) * log_f32(u1)).astype(_F)).astype(_F)
        theta = (_TWO_PI * u2).astype(_F)
        s, c = sincos_f32(theta)
        n1, n2 = (r * c).astype(_F), (r * s).astype(_F)
        out = np.concatenate([n1, n2], axis=-1)
        return fma(out, np.ones_like(out), np.zeros_like(out))     # mean 0, std 1: turns -0 into +0


def normal_from_words(w, E):
    """One draw of ``E`` normals from its ``words(E)`` words."""
    w = np.asarray(w, np.uint32)
    assert w.shape == (words(E),)
    out = np.empty(E, _F)
    full = E - E % 16
    out[:full] = transform16(w[:full].reshape(-1, 16)).reshape(-1)
    if E % 16:
        out[E - 16:] = transform16(w[E:])
    return out


def randn_stream(state_or_seed, draws, E, pos=None):
    """``draws`` consecutive ``torch.randn(E)`` of one stream, fp32 [draws, E], and the stream where it ends."""
    st = state_or_seed.copy() if isinstance(state_or_seed, Stream) else Stream(state_or_seed, pos)
    W = words(E)
    w = st.words(draws * W).reshape(draws, W)
    return np.stack([normal_from_words(w[d], E) for d in range(draws)]) if draws else np.empty((0, E), _F), st


def parse_state(raw):
    """``torch.get_rng_state()`` (5056 bytes) -> Stream.  A generator fresh from ``manual_seed`` (left 1, next 0) holds the
    key and regenerates before its first word, which is position 624 here."""
    b = np.asarray(raw, dtype=np.uint8)
    assert b.shape == (STATE_BYTES,)
    left = int(b[8:12].view(np.int32)[0])
    nxt = int(b[16:24].view(np.uint64)[0])
    state = b[24:24 + 8 * N].view(np.uint64).astype(np.uint32)
    return Stream(state, N if left == 1 else nxt)


def write_state(raw, stream):
    """A copy of ``raw`` with the walk replaced by ``stream``: next = pos and left = 625 - pos, as the generator leaves them
    after it has produced a word; seed, seeded flag and the normal-sample cache stay."""
    b = np.array(raw, dtype=np.uint8)
    assert b.shape == (STATE_BYTES,)
    b[8:12] = np.array([N + 1 - stream.pos], np.int32).view(np.uint8)
    b[16:24] = np.array([stream.pos], np.uint64).view(np.uint8)
    b[24:24 + 8 * N] = stream.state.astype(np.uint64).view(np.uint8)
    return b
