"""The oracle's stage chain restated in numpy long double (x87 extended: 64-bit significand), CPU only.

Block-exact restatement of run_half, run_dft and run_poly of oracle/rate_oracle.c with the same fifos, block structure,
remL / remM, pre / pre_post / preload, 2^k spectrum replication, Nyquist fold and trims -- not a time-domain equivalent: the
frequency-domain decimation truncates a spectrum, which differs from decimating a linear convolution at the level of the
filter's stop band (~1e-9).  One call pattern: the whole input in one push, then drain (chan_flush: 1024-zero appends until
the output fifo holds the frames that are due, then keep exactly those).

Given data (promoted exactly from fp64) come from the oracle: Oracle.plan(), dft_spectrum(), dft_which(), poly_table(),
half_coefs().  Every operation on samples is long double: FFTs through np.fft (complex256), dot products and Horner steps on
longdouble arrays.  The model shares no arithmetic with the oracle: not its FFT, not its loops.

The case table of the fp64 parity tests (tests/test_chain_ld.py on the CPU, tests/test_gpu_fp64_parity.py on the GPU) lives
here, with a per-process cache of (input, model output, oracle output, e_o) so both files pay for a chain once.
"""
import numpy as np

from oracle_binding import Oracle, lcg_noise

LD = np.longdouble
TWO32 = 1 << 32

_C256 = getattr(np, "complex256", None)
PROBLEM = None
if np.finfo(LD).nmant < 63:
    PROBLEM = "np.longdouble has a %d-bit mantissa here; the long-double chain model needs >= 63" % np.finfo(LD).nmant
elif _C256 is None or np.fft.rfft(np.zeros(8, LD)).dtype != _C256:
    PROBLEM = "np.fft.rfft of a longdouble array is %s here, not complex256" % np.fft.rfft(np.zeros(8, LD)).dtype


def require():
    """Tests that use the model call this first: without extended precision they fail with the reason (they do not skip)."""
    if PROBLEM:
        raise RuntimeError(PROBLEM)


def _unpack(H):
    """Packed real spectrum (a[0] = X0, a[1] = X[N/2], a[2k], a[2k+1] = Re, Im X[k]) -> N/2 + 1 complex bins."""
    N = H.shape[0]
    c = np.empty(N // 2 + 1, _C256)
    c[0], c[N // 2] = H[0], H[1]
    c[1:N // 2] = H[2::2].astype(LD) + 1j * H[3::2].astype(LD)
    return c


class _Stage:
    pass


class ChainLD:
    """The chain of one open Oracle.  run(x) -> long double output [frames_out, nch]."""

    PERTURBATIONS = ("poly_last_tap", "horner_linear", "horner_top", "half_outer", "dft_outer_tap", "twiddle")

    def __init__(self, o):
        require()
        self.factor = float(o.cfg.in_rate) / float(o.cfg.out_rate)
        self.isamp_max = o.isamp_max
        self.stages = []
        for i, p in enumerate(o.plan()):
            s = _Stage()
            s.kind = p["kind"]
            s.pre, s.pre_post, s.preload = p["pre"], p["pre_post"], p["preload"]
            if s.kind == "half":
                s.hb = o.half_coefs(i).astype(LD)
                assert len(s.hb) == p["n"]
            elif s.kind == "dft":
                which = o.dft_which(i)
                s.N, s.ov, s.L, s.step_int, s.remL0 = p["dft_length"], p["num_taps"] - 1, p["L"], p["step_int"], p["remL"]
                s.H = _unpack(o.dft_spectrum(which))
                s.taps = o.dft_taps(which)
                assert s.H.shape[0] == s.N // 2 + 1
            else:
                s.n, s.order, s.phase_bits, s.L = p["n"], p["interp_order"], p["phase_bits"], p["L"]
                s.at0, s.step, s.out_in_ratio = p["at"], p["step"], p["out_in_ratio"]
                tab = o.poly_table().astype(LD)
                s.tab = tab.reshape(-1, s.n, s.order + 1)  # [phase][tap][order + 1], highest power first
            self.stages.append(s)

    def has(self, what):
        kinds = [s.kind for s in self.stages]
        if what == "half_outer":
            return "half" in kinds
        if what in ("dft_outer_tap", "twiddle"):
            return "dft" in kinds
        if what == "poly_last_tap":
            return "poly" in kinds
        order = max([s.order for s in self.stages if s.kind == "poly"] or [0])
        return order >= (2 if what == "horner_top" else 1)

    # ---- stage functions: fifo in (nch, count) -> appended to out ----
    @staticmethod
    def _half(s, st, hb):
        x = st["in"]
        avail = max(0, x.shape[1] - s.pre_post)
        num_out = (avail + 1) // 2
        if not num_out:
            return x[:, :0]
        c = s.pre
        y = x[:, c:c + 2 * num_out:2] * LD(.5)
        for k in range(len(hb)):
            d = 2 * k + 1
            y = y + (x[:, c - d:c - d + 2 * num_out:2] + x[:, c + d:c + d + 2 * num_out:2]) * hb[k]
        st["in"] = x[:, 2 * num_out:]
        return y

    @staticmethod
    def _dft(s, st, H, twiddle):
        N, ov, L = s.N, s.ov, s.L
        outs = []
        pow2 = L >= 2 and not (L & (L - 1))
        while st["remL"] + L * max(0, st["in"].shape[1]) >= N:
            x = st["in"]
            span = N - ov - st["remL"] + L - 1
            take, take_rem = span // L, span % L
            if pow2:  # the P-point spectrum, periodically extended: zero stuffing by 2^k in the frequency domain
                P = N // L
                Xp = np.conj(np.fft.rfft(x[:, :P], axis=1))
                full = np.concatenate([Xp, np.conj(Xp[:, P // 2 - 1:0:-1])], axis=1)  # bins 0 .. P-1
                X = full[:, np.arange(N // 2 + 1) % P]
            else:
                if L == 1:
                    blk = x[:, :N]
                else:  # time-domain zero stuffing
                    blk = np.zeros((x.shape[0], N), LD)
                    cnt = len(range(st["remL"], N, L))
                    blk[:, st["remL"]::L] = x[:, :cnt]
                    st["remL"] = L - 1 - take_rem
                X = np.conj(np.fft.rfft(blk, axis=1))
            st["in"] = x[:, take:]
            if twiddle is not None and st["blocks"] == twiddle[0]:
                X = X.copy()
                X[:, twiddle[1]] *= twiddle[2]
            st["blocks"] += 1
            if s.step_int > 0:
                y = np.fft.irfft(np.conj(X * H), N, axis=1) * LD(N // 2)
                if s.step_int != 1:  # time-domain decimation
                    idx = np.arange(st["remM"], N - ov, s.step_int)
                    nxt = st["remM"] + len(idx) * s.step_int
                    st["remM"] = nxt - (N - ov)
                    outs.append(y[:, idx])
                else:
                    outs.append(y[:, :N - ov])
            else:  # frequency-domain decimation by 2^m: keep the low Nd/2 bins, fold the new Nyquist bin to its real part
                m = -s.step_int
                Nd = N >> m
                Y = (X * H)[:, :Nd // 2 + 1].copy()
                Y[:, Nd // 2] = Y[:, Nd // 2].real
                y = np.fft.irfft(np.conj(Y), Nd, axis=1) * LD(Nd // 2)
                outs.append(y[:, :N - ((((1 << m) - 1) * N + ov) >> m)])
        return np.concatenate(outs, axis=1) if outs else st["in"][:, :0]

    @staticmethod
    def _poly(s, st, tab, n_used):
        x = st["in"]
        nch = x.shape[0]
        num_in = max(0, x.shape[1] - s.pre_post)
        n = s.n
        taps = np.arange(n_used)
        outs = []
        if s.order == 0:
            at, step = st["at"] >> 32, s.step >> 32
            k = max(0, -((at - num_in * s.L) // step))  # ceil((num_in L - at) / step)
            for c0 in range(0, k, 16384):
                ats = at + step * np.arange(c0, min(k, c0 + 16384), dtype=np.int64)
                X = x[:, (ats // s.L)[:, None] + taps]
                outs.append((X * tab[ats % s.L, :n_used, 0]).sum(axis=2))
            end = at + k * step
            st["in"] = x[:, end // s.L:]
            st["at"] = (end % s.L) << 32
        else:
            at = st["at"]
            k = max(0, -((at - (num_in << 32)) // s.step))
            pb = s.phase_bits
            for c0 in range(0, k, 16384):
                ats = at + s.step * np.arange(c0, min(k, c0 + 16384), dtype=np.int64)
                frac = ats & (TWO32 - 1)
                ph = frac >> (32 - pb)
                t = (((frac << pb) & (TWO32 - 1)).astype(LD) / LD(TWO32))[:, None]
                c = tab[ph, :n_used]
                v = c[..., 0]
                for q in range(1, s.order + 1):
                    v = v * t + c[..., q]
                X = x[:, (ats >> 32)[:, None] + taps]
                outs.append((X * v).sum(axis=2))
            end = at + k * s.step
            st["in"] = x[:, end >> 32:]
            st["at"] = end & (TWO32 - 1)
        return np.concatenate(outs, axis=1) if outs else np.zeros((nch, 0), LD)

    # ---- the call pattern ----
    def run(self, x, perturb=None):
        """x: [frames, nch] float32 or float64.  perturb: one of PERTURBATIONS, applied to the first stage it fits (the model
        only: nothing of the oracle or the product changes)."""
        x = np.asarray(x)
        frames, nch = x.shape
        assert frames <= self.isamp_max, "one push takes at most isamp_max frames"
        par = []
        done = perturb is None
        for s in self.stages:
            p = {"n_used": getattr(s, "n", 0), "twiddle": None}
            if s.kind == "half":
                p["hb"] = s.hb
                if not done and perturb == "half_outer":
                    p["hb"] = s.hb.copy()
                    p["hb"][-1] = 0
                    done = True
            elif s.kind == "dft":
                p["H"] = s.H
                if not done and perturb == "dft_outer_tap":
                    # the outermost nonzero tap alone, placed and scaled as the oracle places it, transformed in long double
                    i = int(np.flatnonzero(s.taps)[0])
                    one = np.zeros(s.N, LD)
                    one[(i + s.N - len(s.taps) + 1) & (s.N - 1)] = LD(s.taps[i]) / s.N * 2 * s.L
                    p["H"] = s.H - np.conj(np.fft.rfft(one))
                    done = True
                if not done and perturb == "twiddle":
                    # one bin of the second block (passband) turned by one step of the N-point twiddle table
                    th = 8 * np.arctan(LD(1)) / s.N
                    M = s.step_int if s.step_int > 0 else 1 << -s.step_int
                    nbin = s.N // (16 * max(s.L, M))
                    p["twiddle"] = (1, max(1, nbin), np.cos(th) + 1j * np.sin(th))
                    done = True
            else:
                p["tab"] = s.tab
                if not done and perturb == "poly_last_tap":
                    p["n_used"] = s.n - 1
                    done = True
                if not done and perturb in ("horner_linear", "horner_top") and s.order >= (2 if perturb == "horner_top" else 1):
                    p["tab"] = s.tab.copy()
                    p["tab"][s.tab.shape[0] // 3, :, s.order - 1 if perturb == "horner_linear" else 0] = 0
                    done = True
            par.append(p)
        assert done, "perturbation %r fits no stage of this chain" % perturb

        state = []
        for s in self.stages:
            st = {"in": np.zeros((nch, s.preload), LD)}
            if s.kind == "dft":
                st.update(remL=s.remL0, remM=0, blocks=0)
            elif s.kind == "poly":
                st["at"] = s.at0
            state.append(st)
        out = np.zeros((nch, 0), LD)

        def process(new):
            nonlocal out
            for s, st, p in zip(self.stages, state, par):
                st["in"] = np.concatenate([st["in"], new], axis=1)
                if s.kind == "half":
                    new = self._half(s, st, p["hb"])
                elif s.kind == "dft":
                    new = self._dft(s, st, p["H"], p["twiddle"])
                else:
                    new = self._poly(s, st, p["tab"], p["n_used"])
            out = np.concatenate([out, new], axis=1)

        process(np.ascontiguousarray(x.T).astype(LD))
        self.blocks_before_drain = [st.get("blocks", 0) for st in state]
        target = int(frames / self.factor + .5)
        zeros = np.zeros((nch, 1024), LD)
        while out.shape[1] < target:
            process(zeros)
        return np.ascontiguousarray(out[:, :target].T)


# ---- the fp64 parity cases -------------------------------------------------------------------------------------------------
BW99 = {"bandwidth": 99.0}
NORM = {"quality": 1}


def distance(y, ref):
    """(max|y - ref| / max|ref|, relative RMS), both in long double."""
    d = np.asarray(y, LD) - ref
    return float(np.abs(d).max() / np.abs(ref).max()), float(np.sqrt((d * d).sum() / (ref * ref).sum()))


def oracle_fp64(o, x):
    """The oracle's fp64 output fifo after one push and a drain, never pulled: [frames_out, nch]."""
    assert o.push(x) == 0 and o.drain() == 0
    ns = len(o.plan())
    return np.stack([o.stage_fifo(ch, ns) for ch in range(o.nch)], axis=1)


_cache = {}
_blocks = {}


def reference(fi, fo, kw, frames, nch, seed=4242):
    """(x float32 [frames, nch], ld [m, nch] long double, o [m, nch] float64, e_o, rms_o), computed once per process."""
    key = (fi, fo, tuple(sorted(kw.items())), frames, nch, seed)
    if key not in _cache:
        x = lcg_noise(frames, nch, seed).reshape(frames, nch)
        o = Oracle(fi, fo, nch, **kw)
        m = ChainLD(o)
        ld = m.run(x)
        _blocks[key] = [(getattr(s, "N", 0), b) for s, b in zip(m.stages, m.blocks_before_drain)]
        ref = oracle_fp64(o, x)
        o.close()
        e_o, rms_o = distance(ref, ld) if ref.shape == ld.shape else (float("inf"), float("inf"))
        for a in (x, ld, ref):
            a.setflags(write=False)
        _cache[key] = (x, ld, ref, e_o, rms_o)
    return _cache[key]


def blocks_before_drain(fi, fo, kw, frames, nch, seed=4242):
    """[(dft length or 0, blocks the stage ran on the pushed input alone)] per stage, from the model's run."""
    reference(fi, fo, kw, frames, nch, seed)
    return _blocks[(fi, fo, tuple(sorted(kw.items())), frames, nch, seed)]


# (id, in_rate, out_rate, options, frames, channels, streams, call pattern).  Frames: the smallest round count that gives at
# least three blocks of the chain's longest DFT stage plus the drain: 12 000 at the first stage's rate for 4096-point blocks,
# scaled with the block length and with the half-band stages in front (test_chain_ld.py asserts the three blocks).
# Channels: 3 (a pair plus a lone channel) where the generic kernels serve the chain, 2 for the lean kernels, which need an
# even count.  Call pattern: "flow" = device flow_device on torch's stream, "push" = host push / pull_all.
CASES = [
    ("44k1_96k_lean", 44100, 96000, {}, 12000, 2, 1, "flow"),         # x2 dft -> vpoly0 160/147, lean fused kernel
    ("44k1_96k_generic", 44100, 96000, {}, 12000, 3, 1, "push"),      # ... generic fused_kernel + seam_kernel
    ("44k1_96k_2x3", 44100, 96000, {}, 12000, 3, 2, "flow"),          # 2 streams x 3 channels
    ("96k_44k1", 96000, 44100, {}, 12000, 3, 1, "flow"),              # L1 dft -> vpoly0 147/320
    ("44k1_192k_bw99_sub", 44100, 192000, BW99, 48000, 2, 1, "flow"),  # 16384 sub-blocked -> x4 dftx
    ("44k1_192k_bw99", 44100, 192000, BW99, 48000, 3, 1, "push"),     # 16384 dft_kernel -> polymf (n 28) -> x4 dftx
    ("44k1_48k_bw99_flow", 44100, 48000, BW99, 48000, 2, 1, "flow"),  # sub-blocked, outputs into the caller's buffer (OMODE 0)
    ("44k1_48k_bw99_push", 44100, 48000, BW99, 48000, 2, 1, "push"),  # ... through the fifo (OMODE 2)
    ("96k_44k1_bw99", 96000, 44100, BW99, 48000, 3, 1, "flow"),       # 16384-point L1 dft_kernel + polymf
    ("88k2_44k1", 88200, 44100, {}, 12000, 3, 1, "flow"),             # frequency-domain /2, single stage
    ("176k4_44k1", 176400, 44100, {}, 24000, 3, 1, "flow"),           # half NC 11 -> frequency-domain /2
    ("384k_44k1", 384000, 44100, {}, 48000, 3, 1, "push"),            # half NC 12 twice -> dft -> vpoly0
    ("192k_44k1_norm", 192000, 44100, NORM, 24000, 3, 1, "flow"),     # half NC 9, 16-tap vpoly0
    ("352k8_44k1_norm", 352800, 44100, NORM, 48000, 3, 1, "flow"),    # half NC 8 twice
    ("32k_96k", 32000, 96000, {}, 24000, 3, 1, "flow"),               # time-domain zero stuffing x3, 8192
    ("48k_32k", 48000, 32000, {}, 24000, 3, 1, "push"),               # L2 M3, time-domain decimation
    ("48k_192k", 48000, 192000, {}, 24000, 3, 1, "flow"),             # x4 dftx alone
    ("44k1_48001", 44100, 48001, {}, 12000, 3, 1, "flow"),            # vpoly3, 24 taps, 8 phase bits
    ("96k_44101_norm", 96000, 44101, NORM, 12000, 3, 1, "flow"),      # vpoly2, 16 taps, 7 phase bits, step > 1
    ("8k_44117_norm", 8000, 44117, NORM, 12000, 3, 1, "push"),        # vpoly2 feeding a 2048-point x4 stage
    ("44k1_11027_norm", 44100, 11027, NORM, 24000, 3, 1, "flow"),     # vpoly1, 12 taps, 11 phase bits (found by the plan sweep)
    ("22k05_8k_bw99", 22050, 8000, BW99, 96000, 3, 1, "flow"),        # 32768 four-step, poly 160/441 behind it
    ("16k_8k_bw997", 16000, 8000, {"bandwidth": 99.7}, 192000, 3, 1, "flow"),   # 65536, frequency-domain /2
    ("44k1_48k_bw999", 44100, 48000, {"bandwidth": 99.9}, 330000, 2, 1, "flow"),  # 131072 x2, poly behind it
    ("44k1_48k_phase25", 44100, 48000, {"phase": 25.0}, 24000, 2, 1, "flow"),   # minimum-phase taps through the same kernels
    ("8k_192k_bw99", 8000, 192000, BW99, 32000, 3, 1, "push"),        # 3-phase vpoly0 behind 16384-point blocks: poly_kernel<0>
    ("8k_352k8", 8000, 352800, {}, 12000, 3, 1, "push"),              # L >= 8 zero-stuffing branch
]
CASE_IDS = [c[0] for c in CASES]


def case_reference(case):
    """reference() of a case: streams are further channels of one oracle handle (channels are independent)."""
    _, fi, fo, kw, frames, nch, S, _ = case
    return reference(fi, fo, kw, frames, nch * S)
