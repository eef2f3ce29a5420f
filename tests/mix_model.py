"""The numpy model of the channel-mixing rule (include/ratelib_amd.h, "Channel mixing"), written from that rule and nothing else:

    v_c = the source sample of channel c as an exact double (s * 2^-15 / 2^-23 / 2^-31, (double)x for float32, x for float64)
    y_o = sum over c ascending of mix[o][c] * v_c, every product and every sum rounded on its own, WITHOUT the terms whose
          coefficient is zero; the sum starts from its first product; a row of zeros gives +0.0
    x_o = (float)y_o for float32 rows, y_o for float64 rows

numpy's elementwise products and sums are one fp64 operation each: nothing is fused."""
import numpy as np

BITS = {16: 15, 24: 23, 32: 31}                              # RRX_FMT_S16 / RRX_FMT_S24_3 / RRX_FMT_S32 -> bits of the scale


def s24_values(raw):
    """packed little-endian three-byte samples (uint8 [..., n * 3]) -> int64 [..., n], sign-extended"""
    b = np.asarray(raw, np.uint8).reshape(raw.shape[:-1] + (-1, 3)).astype(np.int64)
    v = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return np.where(v >= 1 << 23, v - (1 << 24), v)


def exact(raw, fmt):
    """the source as exact doubles [frames, nch_src]: `raw` is what the call takes (float32 / float64 / int16 / int32
    [frames, nch_src], or uint8 [frames, nch_src * 3] for fmt 24)"""
    if fmt == 24:
        return s24_values(raw).astype(np.float64) * 2.0 ** -23
    if fmt in (16, 32):
        return raw.astype(np.float64) * 2.0 ** -BITS[fmt]
    return raw.astype(np.float64)


def mix(v, M, dtype=np.float32):
    """v: float64 [frames, nch_src]; M: [nch_dst, nch_src] -> [frames, nch_dst] of dtype"""
    M = np.asarray(M, np.float64)
    assert v.dtype == np.float64 and v.ndim == 2 and v.shape[1] == M.shape[1]
    y = np.zeros((v.shape[0], M.shape[0]), np.float64)       # (+0.0: what a row of zeros gives)
    with np.errstate(all="ignore"):
        for o in range(M.shape[0]):
            acc = None
            for c in range(M.shape[1]):
                if M[o, c] == 0:
                    continue
                p = M[o, c] * v[:, c]
                acc = p if acc is None else acc + p
            if acc is not None:
                y[:, o] = acc
        return y.astype(dtype)


def mix_raw(raw, fmt, M, dtype=np.float32):
    return mix(exact(raw, fmt), M, dtype)
