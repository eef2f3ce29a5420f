"""A numpy restatement of the loudness arithmetic that include/ratelib_amd.h makes part of the ABI (RRX_loudness_device,
RRX_loudness_gate_device): the two-biquad step, the matrix A and M = A^hop, the carry, the hop energies and the gate.  Every
rounding is one whole-array operation (numpy fuses nothing), vectorised over streams, channels and hops; the serial sums of the
gate are np.cumsum.  Beside it an independent serial reference of the hop energies on scipy.signal.lfilter, which agrees with the
decomposition to rounding, not to the bit."""
import numpy as np

K48 = np.array([1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621])


def step(c, g, s):
    """one frame: g and the four entries of s are arrays of one shape; returns (v, new s)"""
    y = c[0] * g + s[0]
    s0 = (c[1] * g - c[3] * y) + s[1]
    s1 = c[2] * g - c[4] * y
    v = c[5] * y + s[2]
    s2 = (c[6] * y - c[8] * v) + s[3]
    s3 = c[7] * y - c[9] * v
    return v, [s0, s1, s2, s3]


def matrix_a(c):
    a = np.zeros((4, 4))
    for i in range(4):
        e = [np.float64(1.0 if k == i else 0.0) for k in range(4)]
        _, s = step(c, np.float64(0.0), e)
        a[:, i] = s
    return a


def matmul(x, y):
    acc = np.zeros((4, 4))
    for k in range(4):
        acc = acc + x[:, k:k + 1] * y[k:k + 1, :]
    return acc


def power(c, hop):
    a = matrix_a(c)
    r = a.copy()
    for bit in bin(hop)[3:]:  # the bits below the most significant one
        r = matmul(r, r)
        if bit == "1":
            r = matmul(r, a)
    return r


def carry(m, s, z):
    """S' = M S + z on arrays [..., 4]"""
    return np.stack([(((m[i, 0] * s[..., 0] + m[i, 1] * s[..., 1]) + m[i, 2] * s[..., 2]) + m[i, 3] * s[..., 3]) + z[..., i] for i in range(4)], axis=-1)


def gained(x, gain=None):
    """the frames as the call sees them: (double)x * gain[s], or (double)x without a gain"""
    g = x.astype(np.float64)
    return g if gain is None else g * np.asarray(gain, dtype=np.float64)[:, None, None]


def run(c, blocks, s):
    """the step over the last axis of blocks [..., hop] from the states s (four arrays [...]): (energy, end states)"""
    energy = np.zeros(blocks.shape[:-1])
    for i in range(blocks.shape[-1]):
        v, s = step(c, blocks[..., i], s)
        energy = energy + v * v
    return energy, s


def hop_energies(g, c, hop, state=None, every_state=False):
    """RRX_loudness_device on gained frames g [nstreams, frames, nch] (float64): (energy [nstreams, nch, frames // hop],
    state_out [nstreams, nch, 4]); `state` is the state at the first frame, None for +0.0.  every_state: instead of state_out,
    S_0 ... S_n as [nstreams, nch, n + 1, 4] -- S_k is the state_out of a call that ends behind hop k - 1, and the first k
    energies are that call's."""
    ns, frames, nch = g.shape
    n = frames // hop
    s = np.zeros((ns, nch, 4)) if state is None else np.array(state, dtype=np.float64)
    if not n:
        return np.zeros((ns, nch, 0)), s[:, :, None] if every_state else s
    blocks = np.ascontiguousarray(g[:, :n * hop].reshape(ns, n, hop, nch).transpose(0, 3, 1, 2))  # [ns, nch, n, hop]
    _, z = run(c, blocks, [np.zeros((ns, nch, n)) for _ in range(4)])
    z = np.stack(z, axis=-1)  # [ns, nch, n, 4]
    m = power(c, hop)
    starts = np.zeros((ns, nch, n + 1, 4))
    for k in range(n):
        starts[:, :, k] = s
        s = carry(m, s, z[:, :, k])
    starts[:, :, n] = s
    energy, _ = run(c, blocks, [starts[:, :, :n, i] for i in range(4)])
    return energy, starts if every_state else s


def serial_energies(g, c, hop):
    """the hop energies of the plain serial filter (scipy.signal.lfilter, from rest), [nstreams, nch, frames // hop]"""
    from scipy.signal import lfilter
    ns, frames, nch = g.shape
    n = frames // hop
    y = lfilter(c[0:3], [1.0, c[3], c[4]], g, axis=1)
    v = lfilter(c[5:8], [1.0, c[8], c[9]], y, axis=1)
    sq = (v * v)[:, :n * hop].reshape(ns, n, hop, nch)
    return sq.sum(axis=2).transpose(0, 2, 1)


def gate_thresholds(abs_lufs=-70.0, rel_lu=-10.0):
    return 10.0 ** ((abs_lufs + 0.691) / 10.0), 10.0 ** (rel_lu / 10.0)


def gate(energy, hop, hops=None, weights=None, abs_threshold=None, rel_factor=None):
    """RRX_loudness_gate_device on energy [nstreams, nch, nhops]: [nstreams, 4] = S2, N2, S1, N1"""
    if abs_threshold is None:
        abs_threshold, rel_factor = gate_thresholds()
    ns, nch, nh = energy.shape
    inv = np.float64(1.0) / (np.float64(4.0) * np.float64(hop))
    out = np.zeros((ns, 4))
    for s in range(ns):
        n = nh if hops is None else min(int(hops[s]), nh)
        if n < 4:
            continue
        e = energy[s, :, :n]
        q = ((e[:, 0:n - 3] + e[:, 1:n - 2]) + e[:, 2:n - 1]) + e[:, 3:n]
        acc = np.zeros(n - 3)
        for ch in range(nch):
            acc = acc + (q[ch] if weights is None else np.float64(weights[ch]) * q[ch])
        with np.errstate(invalid="ignore", divide="ignore"):
            z = acc * inv
            m1 = z > abs_threshold
            s1 = np.cumsum(z[m1])[-1] if m1.any() else np.float64(0.0)
            n1 = np.float64(m1.sum())
            t = np.float64(rel_factor) * (np.float64(s1) / n1)
            m2 = m1 & (z > t)
            s2 = np.cumsum(z[m2])[-1] if m2.any() else np.float64(0.0)
        out[s] = (s2, m2.sum(), s1, n1)
    return out


def lufs(result):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(result[:, 1] > 0, -0.691 + 10.0 * np.log10(result[:, 0] / np.maximum(result[:, 1], 1.0)), -np.inf)
