"""NumPy restatement of the device noise generator (framedipt_amd/csrc/philox.hpp; contract in include/fdipt.h) — test infrastructure.

Philox4x32-10 (Salmon et al., SC'11) -> two 53-bit uniforms per call -> Box-Muller in float64.  Key = the sample's 64-bit noise key
(low word, high word); counter = (residue index i, step index k, purpose, call index j); j = 0 gives components x, y and j = 1 gives z.
``distribution_report`` holds the statistical bounds of the distribution tests, so that the CPU test of this restatement and the GPU test
of the device code ask exactly the same thing.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four integer arrays (or scalars) of one shape; key: a Python int < 2^64.  -> four uint64 arrays holding 32-bit words."""
    c = [np.asarray(x).astype(np.uint64) & _MASK for x in np.broadcast_arrays(*counter)]
    k0, k1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]  # 32 x 32 -> 64 bit products
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def uniform53(a, b):
    """((a >> 5) * 2^26 + (b >> 6) + 0.5) * 2^-53 in (0, 1); every operation is exact in float64."""
    return ((a >> np.uint64(5)).astype(np.float64) * 2.0 ** 26 + (b >> np.uint64(6)).astype(np.float64) + 0.5) * 2.0 ** -53


def normals(keys, purpose, k_begin, n_steps, N):
    """[n_steps, B, N, 3] float64: what fdipt_noise_fill(B, N, keys, purpose, k_begin, n_steps) writes."""
    keys = [int(k) & 0xFFFFFFFFFFFFFFFF for k in np.asarray(keys, dtype=object).reshape(-1)]
    k, i = np.meshgrid(np.arange(k_begin, k_begin + n_steps), np.arange(N), indexing="ij")
    out = np.empty((n_steps, len(keys), N, 3))
    for b, key in enumerate(keys):
        for j in range(2):
            w = philox4x32_10((i, k, purpose, j), key)
            r = np.sqrt(-2.0 * np.log(uniform53(w[0], w[1])))
            a = 6.283185307179586 * uniform53(w[2], w[3])
            if j == 0:
                out[:, b, :, 0], out[:, b, :, 1] = r * np.cos(a), r * np.sin(a)
            else:
                out[:, b, :, 2] = r * np.cos(a)  # (its second normal is discarded)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Distribution bounds.  alpha = 1e-9 per statistic and fixed keys: the tests are deterministic, and a correct generator would fail one
# statistic with probability about alpha had the keys been drawn at random.  Every bound follows from n, the number of values (or pairs)
# the statistic really uses; none is tuned to what the generator gives.
ALPHA = 1e-9
DIST_KEYS = tuple(range(1000, 1008))       # consecutive keys: samples b and b + 1
DIST_BIT_KEYS = (1000, 1000 ^ (1 << 40))   # two keys that differ in one bit
DIST_T, DIST_N = 500, 300


def _corr(x, y):
    return abs(float(np.corrcoef(np.ravel(x), np.ravel(y))[0, 1])), int(np.size(x))


def distribution_report(z, other, bit_pair):
    """z [T,B,N,3]: one purpose's draws for DIST_KEYS; other: the paired purpose's draws (rotation against translation of the same
    (k, i)); bit_pair [T,2,N,3]: the same purpose for DIST_BIT_KEYS.  -> list of (name, value, bound); every value must be below its bound."""
    from scipy import stats
    q = float(stats.norm.isf(ALPHA / 2))
    n = z.size
    flat = np.sort(z.ravel())
    cdf = stats.norm.cdf(flat)
    ks = max(float(np.max(np.arange(1, n + 1) / n - cdf)), float(np.max(cdf - np.arange(0, n) / n)))
    rows = [("ks", ks, float(np.sqrt(np.log(2 / ALPHA) / (2 * n)))),  # Dvoretzky-Kiefer-Wolfowitz
            ("mean", abs(float(z.mean())), q / np.sqrt(n)),
            ("var", abs(float(z.var()) - 1.0), q * np.sqrt(2.0 / n))]
    for name, (c, m) in (("corr rot/trans", _corr(z, other)), ("corr step k/k+1", _corr(z[:-1], z[1:])),
                         ("corr residue i/i+1", _corr(z[:, :, :-1], z[:, :, 1:])), ("corr x/y", _corr(z[..., 0], z[..., 1])),
                         ("corr sample b/b+1", _corr(z[:, :-1], z[:, 1:])), ("corr one-bit keys", _corr(bit_pair[:, 0], bit_pair[:, 1]))):
        rows.append((name, c, q / np.sqrt(m)))
    return rows
