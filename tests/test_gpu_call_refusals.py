"""The call checks the blocks share (csrc/call_checks.h) through the real C ABI, one table row per entry point -- vit, reed
and ldpc (rows), burst and ofdm (windows), mod and ofdmmod (frames) at the shapes of the blocks' own
test_refusals_launch_nothing; chan, ddc, psd, iir, polar, beam and cov (streams) and the four that keep their own
sequence (combine, corr, mvdr, eig) at the smallest shapes they accept, their good call held to a fresh handle's bits.
A stride that would wrap a byte range is sent only to the entry points that have always refused it (the burst chain,
polar); for the others the rule is asserted on the host, through the functions the entry points call
(tests/host/test_call_checks.cpp), since a build without it would launch the call.
Each shared rule refuses one bad call with its return code and the WHOLE message: the
prefix and the block's nouns are wired per entry point, and only the whole text tells a swap.  The outputs are poisoned
before the refused calls and bit-identical after them; then one good call gives the block's plan bit for bit (burst and
ofdm, whose plans are float64 twins held to a tolerance by their own tests: a fresh handle through the wrapper).  The
format setters that are one rule each get a row too.  The FIR and the resample / decimate handles have a table of their
own below (the channel family: fir_process_stream, fir_calibrate, rs_process_stream; and the two load_history): these gained
the refusal of a wrapped stride, and fir_calibrate its alignment and overlap rules, together with the rows, so those are
sent too.  Every bad call is refused on the host before any launch.  `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import ldpc_cases as lc
import mod_checks as mchk
import ofdm_cases as oc
import ofdmmod_cases as omc
import reed_cases as rc
from simplefe_amd import synth
from vit_cases import rows_of

pytestmark = pytest.mark.gpu
F32 = np.float32
POISON = 0x7FD5A5A5
T31 = 1 << 31

NULL = "%s: null buffer"
HUGE = "%s: a stride is so large that its buffer's byte range reaches 2^62"
ALIGN = "%s: buffers must be aligned to their element (%s)"
IN_OUT = "%s: input and output ranges overlap (in-place operation is not supported)"
OUT_OUT = "%s: the output ranges overlap one another"
STARTS = "%s: start_base + b * start_step must stay within +-(2^63 - 2^33) for every burst"
WINDOW_ELEMENTS = "cf32 8 B, u8 (I,Q) pairs 2 B, indices, gates, records and statuses 4 B"


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


def _poisoned(api, n_words):
    return api.DeviceArray.from_numpy(np.full(n_words, POISON, np.uint32).view(F32))


def _words(d, n=None):
    return d.to_numpy(n).view(np.uint32)


class Entry:
    """One entry point: its function, the names of its arguments between the handle and the counter, one good call, the
    poisoned outputs, the refused calls as (overrides, return code, whole message), and what the good call must give."""

    def __init__(self, L, who, handle, order, good, outs, bad, counted, check, keep=()):
        self.fn = getattr(L.load(), "sfe_dsp_" + who)
        self.who, self.handle, self.order, self.good, self.outs, self.bad, self.counted, self.check, self.keep = (
            who, handle, order, good, outs, bad, counted, check, keep)

    def call(self, k, **over):
        a = dict(self.good, **over)
        return self.fn(a.pop("hh", self.handle._h), *[a[name] for name in self.order], C.byref(k), None)


def _rows_bad(who, count, elements, short_in, short_out, g, d_in, in_bytes, d_si, d_out, out_bytes, d_rec, decode, sym=None):
    """The refusals of a row codec: g the good call, in_bytes and out_bytes the extents of its input and output."""
    n = g["n"]
    bad = [(dict(n=T31), -1, "%s: %s = 2147483648 must be below 2^31 per call" % (who, count)),
           (dict(pi=None), -1, NULL % who), (dict(po=None), -1, NULL % who),
           (dict(istride=g["istride"] - 1), -6, short_in), (dict(ostride=g["ostride"] - 1), -6, short_out),
           (dict(istride=1 << 62), -1, HUGE % who), (dict(ostride=1 << 62), -1, HUGE % who),
           (dict(po=d_in.ptr + in_bytes - 1), -1, IN_OUT % who), (dict(pi=d_out.ptr + 8 * ((out_bytes - 1) // 8)), -1, IN_OUT % who)]
    if decode:
        al = ALIGN % (who, elements)
        bad += [(dict(psi=d_si.ptr + 2), -1, al), (dict(pr=d_rec.ptr + 2), -1, al), (dict(ps=g["ps"] + 1), -1, al),
                (dict(pr=d_in.ptr), -1, IN_OUT % who), (dict(ps=d_si.ptr + 4 * (n - 1)), -1, IN_OUT % who),
                (dict(pr=d_out.ptr + 4), -1, OUT_OUT % who), (dict(ps=d_out.ptr + 4 * ((out_bytes - 1) // 4)), -1, OUT_OUT % who),
                (dict(ps=d_rec.ptr + 4), -1, OUT_OUT % who)]
    if sym:
        bad += sym
    return bad


DEC = ("pi", "istride", "psi", "n", "po", "ostride", "pr", "ps")
ENC = ("pi", "istride", "n", "po", "ostride")


def _decoder(api, L, who, h, count, elements, short_in, short_out, x_floats_or_bytes, in_bytes, istride, ostride, n, rec_words, want, sym=None):
    d_in = x_floats_or_bytes
    d_si = api.DeviceArray.from_numpy(np.zeros(64, F32))
    d_out, d_rec, d_st = (_poisoned(api, 256) for _ in range(3))
    g = dict(pi=d_in.ptr, istride=istride, psi=d_si.ptr, n=n, po=d_out.ptr, ostride=ostride, pr=d_rec.ptr, ps=d_st.ptr)
    bad = _rows_bad(who, count, elements, short_in, short_out, g, d_in, in_bytes, d_si, d_out, n * ostride, d_rec, True, sym)

    def check():
        assert np.array_equal(d_out.to_numpy().view(np.uint8)[:n * ostride].reshape(n, ostride), want[0])
        assert np.array_equal(_words(d_rec, rec_words * n).reshape(n, rec_words), want[1])
        assert np.array_equal(d_st.to_numpy(n).view(np.int32), want[2])

    return Entry(L, who, h, DEC, g, [d_out, d_rec, d_st], bad, n, check, keep=(d_in, d_si))


def _encoder(api, L, who, h, count, short_in, short_out, rows, istride, ostride, n, want):
    d_in = api.DeviceArray.from_bytes(np.concatenate([rows.ravel(), np.zeros(64, np.uint8)]))
    d_out = _poisoned(api, 256)
    g = dict(pi=d_in.ptr, istride=istride, n=n, po=d_out.ptr, ostride=ostride)
    bad = _rows_bad(who, count, None, short_in, short_out, g, d_in, n * istride, None, d_out, n * ostride, None, False)

    def check():
        assert np.array_equal(d_out.to_numpy().view(np.uint8)[:n * ostride].reshape(n, ostride), want)

    return Entry(L, who, h, ENC, g, [d_out], bad, n, check, keep=(d_in,))


def _vit(api, L):
    K, gen, n_info, nb = 7, (0o171, 0o133), 64, 3
    h = api.Vit(K, gen, n_info)
    hb = api.Vit(K, gen, n_info, in_mode=L.VIT_IN_BPSK, skip=4)
    assert (h.n_soft, h.n_bytes) == (140, 8)
    x = rows_of(api, K, gen, n_info, None, True, nb, 41)
    who = "vit_process_stream"
    el = "soft values 4 B, symbols 8 B, records and statuses 4 B"
    d_in = api.DeviceArray.from_numpy(np.concatenate([x.ravel(), np.zeros(64, F32)]))
    sym = [(dict(pi=d_in.ptr + 2), -1, ALIGN % (who, el)), (dict(hh=hb._h, pi=d_in.ptr + 4, istride=144), -1, ALIGN % (who, el)),
           (dict(hh=hb._h, istride=143), -6, "vit_process_stream: in_stride 143 < the 144 elements of a burst's row, or out_stride 8 < ceil(n_info / 8) = 8")]
    e = _decoder(api, L, who, h, "n_bursts", el,
                 "vit_process_stream: in_stride 139 < the 140 elements of a burst's row, or out_stride 8 < ceil(n_info / 8) = 8",
                 "vit_process_stream: in_stride 140 < the 140 elements of a burst's row, or out_stride 7 < ceil(n_info / 8) = 8",
                 d_in, 4 * nb * 140, 140, 8, nb, 2, api.vit_plan(K, gen, n_info, x=x), sym)
    e.keep += (hb,)
    return e


def _reed_parts(api):
    shape, nf = rc.SHAPES["C"], 3
    frames, wh = rc.many("C", nf)
    h = api.Reed(*shape, whiten=wh)
    assert (h.payload_bytes, h.frame_bytes) == (96, 120)
    return shape, nf, frames, wh, h


def _reed(api, L):
    shape, nf, frames, wh, h = _reed_parts(api)
    d_in = api.DeviceArray.from_bytes(np.concatenate([frames.ravel(), np.zeros(64, np.uint8)]))
    return _decoder(api, L, "reed_process_stream", h, "n_frames", "records and statuses 4 B; payloads and frames need none",
                    "reed_process_stream: in_stride 119 < the 120 bytes read per frame, or out_stride 96 < the 96 bytes written per frame",
                    "reed_process_stream: in_stride 120 < the 120 bytes read per frame, or out_stride 95 < the 96 bytes written per frame",
                    d_in, nf * 120, 120, 96, nf, 2, api.reed_plan(*shape, whiten=wh, data=frames))


def _reed_enc(api, L):
    shape, nf, frames, wh, h = _reed_parts(api)
    pay = api.reed_plan(*shape, whiten=wh, data=frames)[0]
    return _encoder(api, L, "reed_encode_stream", h, "n_frames",
                    "reed_encode_stream: in_stride 95 < the 96 bytes read per frame, or out_stride 120 < the 120 bytes written per frame",
                    "reed_encode_stream: in_stride 96 < the 96 bytes read per frame, or out_stride 119 < the 120 bytes written per frame",
                    pay, 96, 120, nf, api.reed_plan(*shape, whiten=wh, data=pay, encode=True))


LDPC_ELEMENTS = "soft values 4 B, symbols 8 B, records and statuses 4 B; payloads and codewords need none"


def _ldpc_parts(api):
    s, Z = lc.CASES["B"]
    h = api.Ldpc(s, Z, lc.SCALE, 12, 0, 32)
    assert (h.n, h.k_bytes, h.n_bytes) == (648, 41, 81)
    return s, Z, 3, h


def _ldpc(api, L):
    s, Z, nw, h = _ldpc_parts(api)
    hq = api.Ldpc(s, Z, lc.SCALE, 12, 0, 32, in_mode=L.VIT_IN_QPSK, skip=4)
    x = lc.many("B", nw)
    who = "ldpc_process_stream"
    d_in = api.DeviceArray.from_numpy(np.concatenate([x.ravel(), np.zeros(64, F32)]))
    sym = [(dict(pi=d_in.ptr + 2), -1, ALIGN % (who, LDPC_ELEMENTS)), (dict(hh=hq._h, pi=d_in.ptr + 4, istride=328), -1, ALIGN % (who, LDPC_ELEMENTS)),
           (dict(hh=hq._h, istride=327), -6,
            "ldpc_process_stream: in_stride 327 < the 328 elements read per codeword, or out_stride 41 < the 41 bytes written per codeword")]
    e = _decoder(api, L, who, h, "n_words", LDPC_ELEMENTS,
                 "ldpc_process_stream: in_stride 647 < the 648 elements read per codeword, or out_stride 41 < the 41 bytes written per codeword",
                 "ldpc_process_stream: in_stride 648 < the 648 elements read per codeword, or out_stride 40 < the 41 bytes written per codeword",
                 d_in, 4 * nw * 648, 648, 41, nw, 3, api.ldpc_plan(s, Z, lc.SCALE, 12, 0, 32, x=x), sym)
    e.keep += (hq,)
    return e


def _ldpc_enc(api, L):
    s, Z, nw, h = _ldpc_parts(api)
    pay = api.ldpc_plan(s, Z, lc.SCALE, 12, 0, 32, x=lc.many("B", nw))[0]
    return _encoder(api, L, "ldpc_encode_stream", h, "n_words",
                    "ldpc_encode_stream: in_stride 40 < the 41 elements read per codeword, or out_stride 81 < the 81 bytes written per codeword",
                    "ldpc_encode_stream: in_stride 41 < the 41 elements read per codeword, or out_stride 80 < the 81 bytes written per codeword",
                    pay, 41, 81, nw, api.ldpc_plan(s, Z, data=pay))


WIN = ("pi", "n_in", "in_stride", "px", "xstride", "pg", "gstride", "n_bursts", "base", "step", "po", "ostride")


def _windows(api, L, who, h, fresh, x, row, row_name, base, chan_row):
    """burst (chan_row 0) and ofdm: S = 2 streams of n samples, 3 windows each."""
    S, nb = x.shape[0], 3
    n = x.shape[1]
    d_in = api.DeviceArray.from_numpy(np.concatenate([x.view(F32).ravel(), np.zeros(64, F32)]))
    d_idx, d_gate = api.DeviceArray.from_numpy(np.zeros(S * nb + 8, F32)), api.DeviceArray.from_numpy(np.ones(S * nb + 8, F32))
    words = S * nb * max(row, chan_row) * 2 + 64
    d_out, d_ch, d_rec, d_st = (_poisoned(api, words) for _ in range(4))
    order = WIN + (("pc",) if chan_row else ()) + ("pr", "ps", "sstride")
    g = dict(pi=d_in.ptr, n_in=n, in_stride=n, px=d_idx.ptr, xstride=nb, pg=d_gate.ptr, gstride=nb, n_bursts=nb, base=base, step=2, po=d_out.ptr,
             ostride=row, pc=d_ch.ptr, pr=d_rec.ptr, ps=d_st.ptr, sstride=nb)
    al = ALIGN % (who, WINDOW_ELEMENTS)
    short = "%s: out_stride %%d < %s = %d or status_stride %%d < n_bursts = 3" % (who, row_name, row)
    bad = [(dict(n_in=T31, in_stride=T31), -1, "%s: n_in = 2147483648 must be below 2^31 per call" % who),
           (dict(n_bursts=1 << 30, sstride=1 << 30), -1, "%s: n_streams * n_bursts = 2 * 1073741824 must be below 2^31 per call" % who),
           (dict(pi=None), -1, NULL % who), (dict(po=None), -1, NULL % who),
           (dict(ostride=row - 1), -6, short % (row - 1, 3)), (dict(sstride=nb - 1), -6, short % (row, 2)),
           (dict(in_stride=n - 1), -1, "%s: in_stride %d < n_in %d with 2 streams" % (who, n - 1, n)),
           (dict(base=2 ** 63 - 1, step=0), -1, STARTS % who), (dict(base=-2 ** 63, step=0), -1, STARTS % who),
           (dict(base=0, step=2 ** 62), -1, STARTS % who), (dict(base=0, step=-2 ** 62), -1, STARTS % who),
           (dict(in_stride=1 << 61), -1, HUGE % who), (dict(xstride=1 << 62), -1, HUGE % who), (dict(gstride=1 << 62), -1, HUGE % who),
           (dict(ostride=1 << 60), -1, HUGE % who), (dict(sstride=1 << 61), -1, HUGE % who),
           (dict(pi=d_in.ptr + 4), -1, al), (dict(px=d_idx.ptr + 2), -1, al), (dict(pg=d_gate.ptr + 1), -1, al), (dict(po=d_out.ptr + 4), -1, al),
           (dict(pr=d_rec.ptr + 2), -1, al), (dict(ps=d_st.ptr + 3), -1, al),
           (dict(po=d_in.ptr + 8 * (2 * n - 1)), -1, IN_OUT % who), (dict(pr=d_idx.ptr + 4), -1, IN_OUT % who), (dict(ps=d_gate.ptr), -1, IN_OUT % who),
           (dict(pr=d_out.ptr + 8), -1, OUT_OUT % who), (dict(ps=d_out.ptr + 4 * (S * nb * row * 2 - 1)), -1, OUT_OUT % who),
           (dict(ps=d_rec.ptr + 4), -1, OUT_OUT % who)]
    if chan_row:
        bad += [(dict(pc=d_ch.ptr + 4), -1, al), (dict(pc=d_in.ptr), -1, IN_OUT % who), (dict(pc=d_gate.ptr), -1, IN_OUT % who),
                (dict(pc=d_out.ptr + 8 * (S * nb * row - 1)), -1, OUT_OUT % who), (dict(pr=d_ch.ptr + 8 * (S * nb * chan_row - 1)), -1, OUT_OUT % who),
                (dict(ps=d_ch.ptr + 8), -1, OUT_OUT % who)]

    def check():
        want = fresh(x, np.zeros((S, nb)), np.ones((S, nb)))       # symbols, (channel,) record, status
        assert not want[-1].any()
        got = [d_out.to_numpy(S * nb * row * 2)] + ([d_ch.to_numpy(S * nb * chan_row * 2)] if chan_row else []) + [d_rec.to_numpy(S * nb * 8)]
        for a, b in zip(got, want[:-1]):
            assert np.array_equal(a.view(np.uint32), np.ascontiguousarray(b).view(np.uint32).ravel())
        assert np.array_equal(d_st.to_numpy(S * nb).view(np.int32), want[-1].ravel())

    return Entry(L, who, h, order, g, [d_out, d_rec, d_st] + ([d_ch] if chan_row else []), bad, nb, check, keep=(d_in, d_idx, d_gate, d_ch))


def _burst(api, L):
    sps, N, Lp, lag = 4, 32, 8, 1
    n = (N + 2) * sps + 8
    sig = [synth.burst_signal(synth.psk_symbols(n // sps + 2, 4, seed=synth.SEED + s), sps, n, 0, 0.37, 0.013, 0.5, 0.6) for s in (41, 42)]
    pre = synth.psk_symbols(Lp + 2, 4, seed=synth.SEED + 7)[:Lp].astype(np.complex64)
    new = lambda: api.Burst(pre, sps, N, lag, n_streams=2)
    return _windows(api, L, "burst_process_stream", new(), lambda x, idx, gate: new().demodulate(x, idx=idx, gate=gate, start_base=sps, start_step=2),
                    np.stack(sig), N, "n_sym", sps, 0)


def _ofdm(api, L):
    x0, starts, _ = oc.stream("n64")
    n = oc.reach("n64") + 8
    x = np.stack([x0[int(starts[0]):][:n], x0[int(starts[1]):][:n]])
    a = oc.shape_args("n64", 0)
    h = api.Ofdm(n_streams=2, **a)
    return _windows(api, L, "ofdm_process_stream", h, lambda x, idx, gate: api.Ofdm(n_streams=2, **a).receive(x, idx=idx, gate=gate, start_step=2), x,
                    h.n_sym, "n_data * Nd", 0, h.n_fft)


FRM = ("pi", "istride", "n_bursts", "base", "step", "po", "n")
PLACE_2_31 = "%s: n_out = %d and n_bursts = %d must be below 2^31"
PLACE_END = "%s: the last frame ends behind the stream's n_out = %d samples"


def _frames(api, L, who, h, ht, data, F, row, short, range_of, elements, want, extra):
    nb, n_out = 3, 3 * F + 6
    d_in = api.DeviceArray.from_bytes(np.concatenate([data.ravel(), np.zeros(64, np.uint8)]))
    out = _poisoned(api, 2 * n_out + 64)
    g = dict(pi=d_in.ptr, istride=row, n_bursts=nb, base=2, step=F, po=out.ptr, n=n_out)
    bad = [(dict(n=T31), -1, PLACE_2_31 % (who, T31, nb)), (dict(n_bursts=T31), -1, PLACE_2_31 % (who, n_out, T31)),
           (dict(hh=ht._h, n=n_out - 1), -1, "%s: n_out = %d must be even with SFE_FMT_TX10 (whole 5-byte groups)" % (who, n_out - 1)),
           (dict(base=-1), -1, "%s: start_base = -1 must not be negative" % who),
           (dict(step=F - 1), -1, "%s: start_step = %d is below the frame's F = %d samples (frames must not overlap)" % (who, F - 1, F)),
           (dict(base=7), -1, PLACE_END % (who, n_out)), (dict(n=n_out - 5), -1, PLACE_END % (who, n_out - 5)),
           (dict(po=None), -1, NULL % who), (dict(pi=None), -1, NULL % who), (dict(istride=row - 1), -6, short),
           (dict(n_bursts=2, istride=1 << 62), -1, "%s: in_stride is so large that the %s byte range reaches 2^62" % (who, range_of)),
           (dict(po=out.ptr + 4), -1, ALIGN % (who, elements)),
           (dict(po=d_in.ptr + 8 * ((nb * row - 1) // 8)), -1, IN_OUT % who), (dict(pi=out.ptr + 8 * n_out - 1), -1, IN_OUT % who)] + extra

    def check():
        assert np.array_equal(_words(out, 2 * n_out), want(n_out).view(np.uint32))

    return Entry(L, who, h, FRM, g, [out], bad, n_out, check, keep=(d_in, ht))


def _mod(api, L):
    K, gen, n_info, sps = 7, (0o171, 0o133), 64, 4
    taps = mchk.rc_taps(4, 2)
    h, ht = api.Mod(K, gen, n_info, taps, sps, amp=0.5), api.Mod(K, gen, n_info, taps, sps, amp=0.5, out_fmt=L.FMT_TX10)
    assert (h.frame_len, h.n_bytes) == (576, 8)
    data = mchk.payload_bytes(n_info, 3, 41)
    return _frames(api, L, "mod_process_stream", h, ht, data, 576, 8, "mod_process_stream: in_stride 7 < ceil(n_info / 8) = 8", "payloads'",
                   "cf32 output 8 B; TX10 output and payload bytes need none",
                   lambda n_out: api.mod_plan(K, gen, n_info, taps, sps, amp=0.5, data=data, n_out=n_out, start_base=2, start_step=576),
                   [(dict(hh=ht._h, base=3, n=3 * 576 + 8), 0, "")])      # odd starts under TX10: the modulator's own business


def _ofdmmod(api, L):
    args = omc.shape_args("n64", amp=0.5)
    h, ht = api.OfdmMod(**args), api.OfdmMod(**{**args, "out_fmt": L.FMT_TX10})
    hs = api.OfdmMod(**{**args, "in_mode": L.OFDMMOD_IN_SYMBOLS})
    assert (h.frame_len, h.n_in, hs.n_in) == (640, 81, 324)
    who, el = "ofdmmod_process_stream", "cf32 input and output 8 B; TX10 output and coded bytes need none"
    data = omc.rows(args, 3, 41)
    d_sym = api.DeviceArray(2 * 3 * 324 + 4)
    even = "ofdmmod_process_stream: start_base = %d and start_step = %d must be even with SFE_FMT_TX10 (a frame starts on a 5-byte group)"
    e = _frames(api, L, who, h, ht, data, 640, 81, "ofdmmod_process_stream: in_stride 80 < the 81 bytes a burst reads", "input's", el,
                lambda n_out: api.ofdmmod_plan(**args, data=data, n_out=n_out, start_base=2, start_step=640),
                [(dict(hh=ht._h, base=3), -1, even % (3, 640)), (dict(hh=ht._h, base=0, step=641), -1, even % (0, 641)),
                 (dict(hh=hs._h, pi=d_sym.ptr, istride=323), -6, "ofdmmod_process_stream: in_stride 323 < the 324 cf32 symbols a burst reads"),
                 (dict(hh=hs._h, pi=d_sym.ptr + 4, istride=324), -1, ALIGN % (who, el))])
    e.keep += (hs, d_sym)
    return e


STR = ("pi", "n_in", "in_stride", "po", "ostride")
WRAPPED = "%s: the strides take a byte range to 2^62"
BELOW_2_31 = "%s: n_in = %d must be below 2^31 per call"


def _n31(granule):
    """The smallest multiple of a block's granule that is not below 2^31."""
    return -(-T31 // granule) * granule


def _fresh(api, L, e, new, sizes):
    """The good call of entry e on a new handle, into poisoned outputs of its own: their words."""
    f = new()
    fresh = [_poisoned(api, n) for n in sizes]
    k = C.c_size_t(0)
    assert e.call(k, hh=f._h, **dict(zip(e.out_names, (d.ptr for d in fresh)))) == L.SFE_OK and k.value == e.counted
    api.sync()
    return [_words(d) for d in fresh]


def _check_fresh(api, L, e, new, written):
    """e.check: every output holds what a fresh handle writes, bit for bit -- `written` words each, and poison behind."""
    def check():
        want = _fresh(api, L, e, new, [w + 64 for w in written])
        for d, w, n in zip(e.outs, want, written):
            got = _words(d)
            assert np.array_equal(got, w) and (got[:n] != POISON).all() and (got[n:] == POISON).all()
    e.check = check


def _streams(api, L, who, new, x, n, in_rows, need, need_noun, out_rows, osz, elements, counted, named, n31, extra):
    """A member of the streams family: in_rows rows of n cf32 samples (x: the float32 words as uploaded), one good call with
    in_stride = n and out_stride = need.  new(): a handle of this shape; n31: the n_in of the 2^31 rule (None: the block
    has no such rule, and the call would be launched); extra: the block's own rows."""
    h = new()
    d_in = api.DeviceArray.from_numpy(np.concatenate([x, np.zeros(64, F32)]))
    in_b, out_b = in_rows * n * 8, out_rows * need * osz
    d_out = _poisoned(api, out_b // 4 + 64)
    g = dict(pi=d_in.ptr, n_in=n, in_stride=n, po=d_out.ptr, ostride=need)
    al = ALIGN % (who, elements)
    bad = [(dict(pi=None), -1, NULL % who), (dict(po=None), -1, NULL % who),
           (dict(ostride=need - 1), -6, "%s: out_stride %d < %s%d" % (who, need - 1, need_noun, need)),
           (dict(in_stride=n - 1), -1, "%s: in_stride %d < n_in %d" % (who, n - 1, n) + (" with %d streams" % in_rows if named else "")),
           (dict(pi=d_in.ptr + 4), -1, al), (dict(po=d_out.ptr + osz // 2), -1, al),
           (dict(po=d_in.ptr + in_b - osz), -1, IN_OUT % who), (dict(pi=d_out.ptr + 8 * ((out_b - 1) // 8)), -1, IN_OUT % who)] + extra
    if n31:
        bad.append((dict(n_in=n31, in_stride=n31, ostride=n31), -1, BELOW_2_31 % (who, n31)))
    e = Entry(L, who, h, STR, g, [d_out], bad, counted, None, keep=(d_in,))
    e.out_names = ("po",)
    _check_fresh(api, L, e, new, [out_b // 4])
    return e


CF_U8 = "cf32 8 B, u8 (I,Q) pairs 2 B"


def _chan(api, L):
    """M 4, D 4 (and a handle of D 2), 64 outputs, two streams.  chan has no 2^31 rule: such a call is never sent."""
    M, n, who = 4, 256, "chan_process_stream"
    taps = synth.lowpass_taps(4 * M, 1.0 / M)
    half = api.Chan(taps, M, 2, n_streams=2)
    e = _streams(api, L, who, lambda: api.Chan(taps, M, 4, n_streams=2), synth.synth_cf32(2 * n), n, 2, 64, "n_out ", 2 * M, 8, CF_U8, 64, True, None,
                 [(dict(n_in=n + 2, in_stride=n + 2), -1, "chan_process_stream: n_in = 258 is not a multiple of decim = 4"),
                  (dict(hh=half._h, n_in=n + 1, in_stride=n + 1), -1, "chan_process_stream: n_in = 257 is not a multiple of decim = 2"),
                  (dict(hh=half._h), -6, "chan_process_stream: out_stride 64 < n_out 128")])
    e.keep += (half,)
    return e


def _ddc(api, L):
    """D 3, K 2, 64 outputs, two streams.  2^31 is no multiple of 3: the rule is sent the next multiple."""
    D, n, who = 3, 192, "ddc_process_stream"
    taps = synth.lowpass_taps(8 * D, 0.5 / D)
    return _streams(api, L, who, lambda: api.Ddc(taps, D, [0.125, -0.3], n_streams=2), synth.synth_cf32(2 * n), n, 2, 64, "n_out ", 4, 8,
                    "cf32 8 B, real float 4 B, u8 (I,Q) pairs 2 B", 64, True, _n31(D),
                    [(dict(n_in=n + 1, in_stride=n + 1), -1, "ddc_process_stream: n_in = 193 is not a multiple of decim = 3")])


def _psd(api, L):
    """N 256, hop 128, n_avg 2, eight segments: four rows, two streams."""
    N, hop, n, who = 256, 128, 1024, "psd_process_stream"
    w = np.hanning(N).astype(F32)
    return _streams(api, L, who, lambda: api.Psd(w, hop, 2, n_streams=2), synth.synth_cf32(2 * n), n, 2, 4 * N, "n_rows * n_fft = ", 2, 4,
                    CF_U8 + ", float32 rows 4 B", 4, True, _n31(hop),
                    [(dict(n_in=n + 1, in_stride=n + 1), -1, "psd_process_stream: n_in = 1025 is not a multiple of hop = 128")])


def _iir(api, L):
    """One block, two streams."""
    sos = synth.iir_dc_blocker(0.995)
    n, who = api.iir_plan(sos)[0], "iir_process_stream"
    return _streams(api, L, who, lambda: api.Iir(sos, n_streams=2), synth.synth_cf32(2 * n), n, 2, n, "n_in = ", 2, 8, CF_U8 + ", float32 4 B", n, True,
                    _n31(n), [(dict(n_in=n + 1, in_stride=n + 1, ostride=n + 1), -1,
                               "iir_process_stream: n_in = %d is not a multiple of the block = %d" % (n + 1, n))])


def _polar(api, L):
    """FM, two streams of 64 samples.  polar refused a wrapped byte range before the family was shared, so it is sent both."""
    n, who = 64, "polar_process_stream"
    return _streams(api, L, who, lambda: api.Polar(L.POLAR_FM, 0.5, n_streams=2), synth.synth_cf32(2 * n), n, 2, n, "n_in = ", 2, 4,
                    CF_U8 + ", float32 4 B", n, True, T31,
                    [(dict(in_stride=1 << 61), -1, WRAPPED % who), (dict(ostride=1 << 62), -1, WRAPPED % who)])


def _beam(api, L):
    """S 2, B 2, M 1, 64 samples."""
    n, who = 64, "beam_process_stream"
    W = np.array([[1.0, 0.5j], [0.25 - 0.5j, -1.0]], np.complex64)
    return _streams(api, L, who, lambda: api.Beam(W), synth.synth_cf32(2 * n), n, 2, n, "n_in = ", 2, 8, CF_U8, n, False, T31, [])


def _cov(api, L):
    """S 2, M 1, n_avg = the chunk, two rows of (2 S)^2 floats."""
    who = "cov_process_stream"
    T = api.cov_plan(2, 1, 64)[0]
    n = 2 * T
    return _streams(api, L, who, lambda: api.Cov(2, 1, T), synth.synth_cf32(2 * n), n, 2, 32, "n_rows * (2 n_in_streams)^2 = ", 1, 4,
                    CF_U8 + ", float32 rows 4 B", 2, False, _n31(T),
                    [(dict(n_in=n + 1, in_stride=n + 1), -1, "cov_process_stream: n_in = %d is not a multiple of the chunk = %d" % (n + 1, T))])


def _combine(api, L):
    """M 4, D 4, two streams of 64 instants: its own sequence, with the TX10 and 2^31 rules between the shared ones."""
    M, D, n, who = 4, 4, 64, "combine_process_stream"
    taps = synth.lowpass_taps(4 * M, 1.0 / M)
    new = lambda: api.Combiner(taps, M, D, n_streams=2)
    h, ht = new(), new()
    ht.set_output_format(L.FMT_TX10)
    no, in_b, out_b = n * D, 2 * M * n * 8, 2 * n * D * 8
    d_in = api.DeviceArray.from_numpy(np.concatenate([synth.synth_cf32(2 * M * n), np.zeros(64, F32)]))
    d_out = _poisoned(api, out_b // 4 + 64)
    g = dict(pi=d_in.ptr, n_in=n, in_stride=n, po=d_out.ptr, ostride=no)
    al = ALIGN % (who, "cf32 8 B")
    bad = [(dict(pi=None), -1, NULL % who), (dict(po=None), -1, NULL % who),
           (dict(ostride=no - 1), -6, "combine_process_stream: out_stride 255 < n_out 256"),
           (dict(in_stride=n - 1), -1, "combine_process_stream: in_stride 63 < n_in 64"),
           (dict(hh=ht._h, ostride=no + 1), -1, "combine_process_stream: out_stride 257 must be even with SFE_FMT_TX10 (whole 5-byte groups per stream)"),
           (dict(pi=d_in.ptr + 4), -1, al), (dict(po=d_out.ptr + 4), -1, al),
           (dict(n_in=1 << 29, in_stride=1 << 29, ostride=T31), -1,
            "combine_process_stream: a stream's input (4 x 536870912) or output (2147483648) reaches 2^31 samples"),
           (dict(po=d_in.ptr + in_b - 8), -1, IN_OUT % who), (dict(pi=d_out.ptr + out_b - 8), -1, IN_OUT % who)]
    e = Entry(L, who, h, STR, g, [d_out], bad, no, None, keep=(d_in, ht))
    e.out_names = ("po",)
    _check_fresh(api, L, e, new, [out_b // 4])
    return e


def _corr(api, L):
    """Templates of 257 samples, a block of two transform advances, two blocks, two streams: two peak outputs, one metric."""
    K, B, blocks, who = 2, 2 * 3840, 2, "corr_process_stream"
    n, rows = blocks * B, 2 * K
    t = np.stack([synth.synth_cf32(257, ch=100 + k).view(np.complex64) for k in range(K)])
    t = (np.where(t.real >= 0, 1.0, -1.0) + 1j * np.where(t.imag >= 0, 1.0, -1.0)).astype(np.complex64)
    new = lambda: api.Corr(t, B, 1e-6, n_streams=2)
    d_in = api.DeviceArray.from_numpy(np.concatenate([synth.synth_cf32(2 * n), np.zeros(64, F32)]))
    written = [rows * blocks, rows * blocks, rows * n]
    d_val, d_idx, d_met = (_poisoned(api, w + 64) for w in written)
    g = dict(pi=d_in.ptr, n_in=n, in_stride=n, pv=d_val.ptr, px=d_idx.ptr, pstride=blocks, pm=d_met.ptr, mstride=n)
    al = ALIGN % (who, "cf32 8 B, u8 (I,Q) pairs 2 B, outputs 4 B")
    n31 = _n31(B)
    bad = [(dict(n_in=n + 1, in_stride=n + 1), -1, "corr_process_stream: n_in = 15361 is not a multiple of block = 7680"),
           (dict(n_in=n31, in_stride=n31, pstride=n31 // B, mstride=n31), -1, BELOW_2_31 % (who, n31)),
           (dict(pi=None), -1, NULL % who), (dict(pv=None), -1, NULL % who), (dict(px=None), -1, NULL % who),
           (dict(pstride=blocks - 1), -6, "corr_process_stream: peak_stride 1 < n_blocks = 2"),
           (dict(mstride=n - 1), -6, "corr_process_stream: metric_stride 15359 < n_in = 15360"),
           (dict(in_stride=n - 1), -1, "corr_process_stream: in_stride 15359 < n_in 15360 with 2 streams"),
           (dict(pi=d_in.ptr + 4), -1, al), (dict(pv=d_val.ptr + 2), -1, al), (dict(px=d_idx.ptr + 1), -1, al), (dict(pm=d_met.ptr + 3), -1, al),
           (dict(pv=d_in.ptr + 8 * 2 * n - 4), -1, IN_OUT % who), (dict(px=d_in.ptr), -1, IN_OUT % who), (dict(pm=d_in.ptr + 8), -1, IN_OUT % who),
           (dict(pi=d_met.ptr + 8 * ((4 * rows * n - 1) // 8)), -1, IN_OUT % who),
           (dict(px=d_val.ptr + 4 * (rows * blocks - 1)), -1, OUT_OUT % who), (dict(pm=d_idx.ptr), -1, OUT_OUT % who),
           (dict(pv=d_met.ptr + 4 * (rows * n - 1)), -1, OUT_OUT % who)]
    e = Entry(L, who, new(), ("pi", "n_in", "in_stride", "pv", "px", "pstride", "pm", "mstride"), g, [d_val, d_idx, d_met], bad, blocks, None,
              keep=(d_in,))
    e.out_names = ("pv", "px", "pm")
    _check_fresh(api, L, e, new, written)
    return e


def _grams(rows, n2, seed):
    """rows symmetric positive definite matrices of order n2, float32, as one band's input."""
    a = np.random.default_rng(seed).standard_normal((rows, n2, 3 * n2))
    return (a @ a.transpose(0, 2, 1) / (3 * n2) + np.eye(n2)).astype(F32).ravel()


STEER = np.array([[1.0, 1.0j]], np.complex64)       # S 2, B 1, one band


def _mvdr(api, L):
    """S 2, B 1, M 1, two rows: several optional outputs under one compound SFE_ERANGE sentence."""
    who, rows, gram, mat = "mvdr_process_stream", 2, 16, 8
    new = lambda: api.Mvdr(STEER, False, 1e-3)
    d_g = api.DeviceArray.from_numpy(np.concatenate([_grams(rows, 4, 41), np.zeros(64, F32)]))
    written = [rows * mat, rows, rows]
    d_R, d_p, d_s = (_poisoned(api, w + 64) for w in written)
    g = dict(pg=d_g.ptr, n_rows=rows, in_stride=rows * gram, pR=d_R.ptr, ostride=mat, pp=d_p.ptr, pstride=1, ps=d_s.ptr, sstride=1)
    al = ALIGN % (who, "float32 and int32 4 B")
    short = ("mvdr_process_stream: out_stride %d < n_bands * 4 n_beams n_in = 8, power_stride %d < n_bands * n_beams = 1 or "
             "status_stride %d < n_bands = 1")
    bad = [(dict(n_rows=1 << 27, in_stride=T31), -1, "mvdr_process_stream: n_rows = 134217728 must be below 2^31 / (2 n_in)^2 = 134217728 per call"),
           (dict(pg=None), -1, NULL % who), (dict(pR=None), -1, NULL % who),
           (dict(ostride=mat - 1), -6, short % (7, 1, 1)), (dict(pstride=0), -6, short % (8, 0, 1)), (dict(sstride=0), -6, short % (8, 1, 0)),
           (dict(in_stride=rows * gram - 1), -1, "mvdr_process_stream: in_stride 31 < n_rows * (2 n_in)^2 = 32"),
           (dict(pg=d_g.ptr + 2), -1, al), (dict(pR=d_R.ptr + 2), -1, al), (dict(pp=d_p.ptr + 1), -1, al), (dict(ps=d_s.ptr + 3), -1, al),
           (dict(pR=d_g.ptr + 4 * (rows * gram - 1)), -1, IN_OUT % who), (dict(pp=d_g.ptr), -1, IN_OUT % who), (dict(ps=d_g.ptr + 4), -1, IN_OUT % who),
           (dict(pg=d_R.ptr + 4 * (rows * mat - 1)), -1, IN_OUT % who)]
    e = Entry(L, who, new(), ("pg", "n_rows", "in_stride", "pR", "ostride", "pp", "pstride", "ps", "sstride"), g, [d_R, d_p, d_s], bad, rows, None,
              keep=(d_g,))
    e.out_names = ("pR", "pp", "ps")
    _check_fresh(api, L, e, new, written)
    return e


def _eig(api, L):
    """S 2, B 1, M 1, one eigen-beam, two rows."""
    who, rows, gram, n2, mat = "eig_process_stream", 2, 16, 4, 8
    new = lambda: api.Eig(STEER, False, 2, 1)
    d_g = api.DeviceArray.from_numpy(np.concatenate([_grams(rows, 4, 42), np.zeros(64, F32)]))
    written = [rows * n2, rows, rows * mat, rows]
    d_v, d_n, d_e, d_s = (_poisoned(api, w + 64) for w in written)
    g = dict(pg=d_g.ptr, n_rows=rows, in_stride=rows * gram, pv=d_v.ptr, vstride=n2, pn=d_n.ptr, nstride=1, pe=d_e.ptr, estride=mat, ps=d_s.ptr,
             sstride=1)
    al = ALIGN % (who, "float32 and int32 4 B")
    short = ("eig_process_stream: values_stride %d < n_bands * 2 n_in = 4, null_stride %d < n_bands * n_beams = 1, "
             "vectors_stride %d < n_bands * 4 n_vec n_in = 8 or status_stride %d < n_bands = 1")
    bad = [(dict(n_rows=1 << 27, in_stride=T31), -1, "eig_process_stream: n_rows = 134217728 must be below 2^31 / (2 n_in)^2 = 134217728 per call"),
           (dict(pg=None), -1, NULL % who), (dict(pv=None), -1, NULL % who),
           (dict(vstride=n2 - 1), -6, short % (3, 1, 8, 1)), (dict(nstride=0), -6, short % (4, 0, 8, 1)),
           (dict(estride=mat - 1), -6, short % (4, 1, 7, 1)), (dict(sstride=0), -6, short % (4, 1, 8, 0)),
           (dict(in_stride=rows * gram - 1), -1, "eig_process_stream: in_stride 31 < n_rows * (2 n_in)^2 = 32"),
           (dict(pg=d_g.ptr + 2), -1, al), (dict(pv=d_v.ptr + 1), -1, al), (dict(pn=d_n.ptr + 2), -1, al), (dict(pe=d_e.ptr + 3), -1, al),
           (dict(ps=d_s.ptr + 3), -1, al),
           (dict(pv=d_g.ptr + 4 * (rows * gram - 1)), -1, IN_OUT % who), (dict(pn=d_g.ptr), -1, IN_OUT % who), (dict(pe=d_g.ptr + 4 * 8), -1, IN_OUT % who),
           (dict(ps=d_g.ptr + 4), -1, IN_OUT % who), (dict(pg=d_e.ptr + 4 * (rows * mat - 1)), -1, IN_OUT % who)]
    order = ("pg", "n_rows", "in_stride", "pv", "vstride", "pn", "nstride", "pe", "estride", "ps", "sstride")
    e = Entry(L, who, new(), order, g, [d_v, d_n, d_e, d_s], bad, rows, None, keep=(d_g,))
    e.out_names = ("pv", "pn", "pe", "ps")
    _check_fresh(api, L, e, new, written)
    return e


ENTRIES = {"chan_process_stream": _chan, "ddc_process_stream": _ddc, "psd_process_stream": _psd, "iir_process_stream": _iir,
           "polar_process_stream": _polar, "beam_process_stream": _beam, "cov_process_stream": _cov, "combine_process_stream": _combine,
           "corr_process_stream": _corr, "mvdr_process_stream": _mvdr, "eig_process_stream": _eig,
           "vit_process_stream": _vit, "reed_encode_stream": _reed_enc, "reed_process_stream": _reed, "ldpc_encode_stream": _ldpc_enc,
           "ldpc_process_stream": _ldpc, "burst_process_stream": _burst, "ofdm_process_stream": _ofdm, "mod_process_stream": _mod,
           "ofdmmod_process_stream": _ofdmmod}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_shared_rules_refuse_with_the_entry_points_words(api, L, name):
    e = ENTRIES[name](api, L)
    assert e.who == name and (L.SFE_EINVAL, L.SFE_ERANGE) == (-1, -6)
    lib = L.load()
    k = C.c_size_t(7)
    for over, code, text in e.bad:
        if code == L.SFE_OK:            # a call another block of the family refuses: accepted here, and it may write
            continue
        k.value = 7
        assert e.call(k, **over) == code, (over, lib.sfe_dsp_last_error())
        assert lib.sfe_dsp_last_error() == text.encode() and k.value == 0, (over, lib.sfe_dsp_last_error())
    api.sync()
    for d in e.outs:
        assert (_words(d) == POISON).all(), "a refused call wrote"
    assert e.call(k) == L.SFE_OK and k.value == e.counted
    api.sync()
    e.check()
    for over, code, text in e.bad:
        if code == L.SFE_OK:
            assert e.call(k, **over) == L.SFE_OK, (over, lib.sfe_dsp_last_error())
    api.sync()


# ---- the FIR and the resample / decimate handles: the channel family, and the two load_history entry points.  Their argument
# lists differ from the blocks' (no counter, or a rate in front of it), so they have a table of their own: 2 channels of
# n = 1024 cf32, 17 real taps; the resampler at U = 1, rate 2, blksize 4096; load_history with n_prev = 16.
CH_N, CH_PREV = 1024, 16
CH_ALIGN = "cf32 8 B, f32 4 B, u8 (I,Q) pairs 2 B"
FIR_STRIDE = "%s: channel stride smaller than n"
FIR_NULL = "%s: null handle or buffer"
TX10_GROUPS = "%s: 10-bit output packs 4 floats per group: out_stride must keep channels on group boundaries"


class Channels:
    """One entry point of the two handles: new() a handle of the row's shape, call(h, **a) the entry point over it, the good
    call's arguments, the refused calls as (overrides, return code, whole message), and run(h, d_out) what leaves the good
    call's bits in d_out (for load_history: the good call, then a process_stream), `words` float32 words of them."""

    def __init__(self, new, call, good, bad, d_out, words, run=None, keep=()):
        self.new, self.call, self.good, self.bad, self.d_out, self.words, self.keep = new, call, good, bad, d_out, words, keep
        self.run = run or (lambda h, d_out: call(h, **dict(good, po=d_out.ptr)))


def _fir_rows(api, L, who, call):
    """fir_process_stream and fir_calibrate: the same buffers, the same rules, their own prefix."""
    n = CH_N
    taps = synth.lowpass_taps(17, 0.2)
    new = lambda: api.Fir(taps, data_complex=True, n_channels=2)
    ht = new()
    ht.set_output_format(L.FMT_TX10)
    d_in = api.DeviceArray.from_numpy(np.concatenate([synth.synth_cf32(2 * n), np.zeros(64, F32)]))
    d_out = _poisoned(api, 4 * n + 64)
    good = dict(pi=d_in.ptr, po=d_out.ptr, n=n, istride=n, ostride=n)
    al = ALIGN % (who, CH_ALIGN + "; 10-bit output: none")
    bad = [(dict(hh=None), -1, FIR_NULL % who), (dict(pi=None), -1, FIR_NULL % who), (dict(po=None), -1, FIR_NULL % who),
           (dict(istride=n - 1), -1, FIR_STRIDE % who), (dict(ostride=n - 1), -1, FIR_STRIDE % who),
           (dict(istride=1 << 61), -1, WRAPPED % who), (dict(ostride=1 << 62), -1, WRAPPED % who),
           (dict(istride=(1 << 64) - 1), -1, WRAPPED % who),
           (dict(pi=d_in.ptr + 4), -1, al), (dict(po=d_out.ptr + 4), -1, al),
           (dict(hh=ht._h, ostride=n + 1), -1, TX10_GROUPS % who),
           (dict(po=d_in.ptr + 8 * (2 * n - 1)), -1, IN_OUT % who), (dict(pi=d_out.ptr + 8 * (2 * n - 1)), -1, IN_OUT % who),
           (dict(hh=ht._h, po=d_in.ptr + 8 * 2 * n - 1), -1, IN_OUT % who)]
    return Channels(new, call, good, bad, d_out, 4 * n, keep=(d_in, ht))


def _fir_stream(api, L):
    fn = L.load().sfe_dsp_fir_process_stream
    return _fir_rows(api, L, "fir_process_stream", lambda h, hh=0, **a: fn(h._h if hh == 0 else hh, a["pi"], a["po"], a["n"], a["istride"],
                                                                               a["ostride"], None))


def _fir_calibrate(api, L):
    fn = L.load().sfe_dsp_fir_calibrate
    v = C.c_int(0)
    e = _fir_rows(api, L, "fir_calibrate", lambda h, hh=0, **a: fn(h._h if hh == 0 else hh, a["pi"], a["po"], a["n"], a["istride"], a["ostride"],
                                                                   None, C.byref(v)))
    e.bad.append((dict(n=0), -1, FIR_NULL % "fir_calibrate"))
    return e


def _rs_stream(api, L):
    n, cap, who = CH_N, CH_N // 2, "rs_process_stream"          # rate 2 from a fresh state: n / 2 outputs
    taps = synth.lowpass_taps(17, 0.2)
    new = lambda: api.Rs(taps, 1, 4096, data_complex=True, n_channels=2)
    fn = L.load().sfe_dsp_rs_process_stream
    k = C.c_size_t(7)

    def call(h, hh=0, **a):
        k.value = 7
        rc = fn(h._h if hh == 0 else hh, a["pi"], a["n"], a["istride"], a["po"], a["cap"], a["ostride"], a["rate"], C.byref(k), None)
        assert k.value == (n // 2 if rc == L.SFE_OK else 0)
        return rc

    d_in = api.DeviceArray.from_numpy(np.concatenate([synth.synth_cf32(2 * n), np.zeros(64, F32)]))
    d_out = _poisoned(api, 4 * cap + 64)
    good = dict(pi=d_in.ptr, po=d_out.ptr, n=n, istride=n, cap=cap, ostride=cap, rate=2.0)
    al = ALIGN % (who, CH_ALIGN)
    stride = "rs_process_stream: channel stride smaller than the channel (in_stride >= n_in, out_stride >= out_cap)"
    overlap = "rs_process_stream: input and output ranges overlap"
    bad = [(dict(rate=0.5), -1, "rs_process_stream: rate 0.5 not accepted by this mode"),
           (dict(pi=None), -1, NULL % who), (dict(po=None), -1, NULL % who),
           (dict(istride=n - 1), -1, stride), (dict(ostride=cap - 1), -1, stride),
           (dict(istride=1 << 61), -1, WRAPPED % who), (dict(ostride=1 << 62), -1, WRAPPED % who), (dict(ostride=(1 << 64) - 1), -1, WRAPPED % who),
           (dict(pi=d_in.ptr + 4), -1, al), (dict(po=d_out.ptr + 4), -1, al),
           (dict(po=d_in.ptr + 8 * (2 * n - 1)), -1, overlap), (dict(pi=d_out.ptr + 8 * (2 * cap - 1)), -1, overlap)]
    return Channels(new, call, good, bad, d_out, 4 * cap, keep=(d_in,))


def _load_history(api, L, who, new, process, words):
    """n_prev = 16 samples in front of the stream; the state they leave shows in the process_stream behind them."""
    n = CH_N
    fn = getattr(L.load(), "sfe_dsp_" + who)
    d_prev = api.DeviceArray.from_numpy(np.concatenate([synth.synth_cf32(2 * CH_PREV, ch=7), np.zeros(64, F32)]))
    d_in = api.DeviceArray.from_numpy(np.concatenate([synth.synth_cf32(2 * n), np.zeros(64, F32)]))
    d_out = _poisoned(api, 4 * n + 64)
    good = dict(pp=d_prev.ptr, n_prev=CH_PREV, stride=CH_PREV)
    call = lambda h, hh=0, **a: fn(h._h if hh == 0 else hh, a["pp"], a["n_prev"], a["stride"], None)
    bad = [(dict(hh=None), -1, FIR_NULL % who), (dict(pp=None), -1, FIR_NULL % who),
           (dict(stride=CH_PREV - 1), -1, "%s: channel stride smaller than n_prev" % who),
           (dict(pp=d_prev.ptr + 4), -1, ALIGN % (who, "cf32 8 B, f32 4 B"))]

    def run(h, out):
        assert call(h, **good) == L.SFE_OK
        return process(h, d_in, out, n)

    e = Channels(new, call, good, bad, d_out, words, run, keep=(d_prev, d_in))
    e.process = lambda h, out: process(h, d_in, out, n)
    return e


def _fir_load_history(api, L):
    taps = synth.lowpass_taps(17, 0.2)
    fn = L.load().sfe_dsp_fir_process_stream
    return _load_history(api, L, "fir_load_history", lambda: api.Fir(taps, data_complex=True, n_channels=2),
                         lambda h, d_in, out, n: fn(h._h, d_in.ptr, out.ptr, n, n, n, None), 4 * CH_N)


def _rs_load_history(api, L):
    taps = synth.lowpass_taps(17, 0.2)
    fn = L.load().sfe_dsp_rs_process_stream
    k = C.c_size_t(0)
    return _load_history(api, L, "rs_load_history", lambda: api.Rs(taps, 1, 4096, data_complex=True, n_channels=2),
                         lambda h, d_in, out, n: fn(h._h, d_in.ptr, n, n, out.ptr, n // 2, n // 2, 2.0, C.byref(k), None), 2 * CH_N)


CHANNELS = {"fir_process_stream": _fir_stream, "fir_calibrate": _fir_calibrate, "rs_process_stream": _rs_stream,
            "fir_load_history": _fir_load_history, "rs_load_history": _rs_load_history}


@pytest.mark.parametrize("name", list(CHANNELS))
def test_fir_and_rs_refuse_with_the_entry_points_words(api, L, name):
    """Each rule of the channel family (csrc/call_checks.h: check_channels) and of load_history (csrc/block.h) refuses one
    bad call with its code and whole message, the wrapped strides and fir_calibrate's alignment and overlap rules among
    them; nothing is written and no state moves; then the good call gives a fresh handle's bits."""
    e = CHANNELS[name](api, L)
    lib = L.load()
    h = e.new()
    d_out = e.d_out
    for over, code, text in e.bad:
        assert e.call(h, **dict(e.good, **over)) == code, (over, lib.sfe_dsp_last_error())
        assert lib.sfe_dsp_last_error() == text.encode(), (over, lib.sfe_dsp_last_error())
    api.sync()
    assert (_words(d_out) == POISON).all(), "a refused call wrote"
    fresh = _poisoned(api, len(_words(d_out)))
    if name.endswith("load_history"):
        # the refused calls left the carried state alone: the stream behind them starts from zeros, as a new handle's does
        untouched = _poisoned(api, len(_words(d_out)))
        assert e.process(h, untouched) == L.SFE_OK and e.process(e.new(), fresh) == L.SFE_OK
        api.sync()
        assert np.array_equal(_words(untouched), _words(fresh))
        h = e.new()
    assert e.run(h, d_out) == L.SFE_OK and e.run(e.new(), fresh) == L.SFE_OK
    api.sync()
    got = _words(d_out)
    assert np.array_equal(got, _words(fresh)) and (got[:e.words] != POISON).all() and (got[e.words:] == POISON).all()
    if name.endswith("load_history"):       # and the halo counts: not the bits of a stream that starts from zeros
        assert not np.array_equal(got, _words(untouched))


def _setters(api):
    """(prefix, a handle at a small shape, the setter, the second format's name and value)"""
    lp = synth.lowpass_taps(16, 0.25)
    w = np.hanning(256).astype(F32)
    tpl = np.ones(13, np.complex64)
    a = oc.shape_args("n64", 0)
    pre = synth.psk_symbols(10, 4, seed=synth.SEED + 7)[:8].astype(np.complex64)
    return [("chan", lambda: api.Chan(lp, 4, 4), "set_input_format", "SFE_FMT_U8", 1),
            ("ddc", lambda: api.Ddc(synth.lowpass_taps(24, 0.5 / 3), 3, [0.125, -0.3]), "set_input_format", "SFE_FMT_U8", 1),
            ("psd", lambda: api.Psd(w, 128, 2), "set_input_format", "SFE_FMT_U8", 1),
            ("corr", lambda: api.Corr(tpl, 3840), "set_input_format", "SFE_FMT_U8", 1),
            ("iir", lambda: api.Iir(synth.iir_dc_blocker(0.995)), "set_input_format", "SFE_FMT_U8", 1),
            ("beam", lambda: api.Beam(np.ones((2, 3), np.complex64)), "set_input_format", "SFE_FMT_U8", 1),
            ("cov", lambda: api.Cov(2), "set_input_format", "SFE_FMT_U8", 1),
            ("burst", lambda: api.Burst(pre, 4, 32, 1), "set_input_format", "SFE_FMT_U8", 1),
            ("ofdm", lambda: api.Ofdm(**a), "set_input_format", "SFE_FMT_U8", 1),
            ("combine", lambda: api.Combiner(lp, 4, 4), "set_output_format", "SFE_FMT_TX10", 2)]


@pytest.mark.parametrize("row", range(10), ids=["chan", "ddc", "psd", "corr", "iir", "beam", "cov", "burst", "ofdm", "combine"])
def test_format_setters(api, L, row):
    """A format outside the two allowed, and a null handle: SFE_EINVAL with the setter's sentence; each allowed one: SFE_OK."""
    prefix, new, setter, other_name, other = _setters(api)[row]
    assert (L.FMT_F32, getattr(L, other_name[4:])) == (0, other)
    lib = L.load()
    fn = getattr(lib, "sfe_dsp_%s_%s" % (prefix, setter))
    text = ("%s_%s: null handle or a format other than SFE_FMT_F32 / %s" % (prefix, setter, other_name)).encode()
    h = new()
    for fmt in (3 - other, 3, -1):
        assert fn(h._h, fmt) == L.SFE_EINVAL and lib.sfe_dsp_last_error() == text, (fmt, lib.sfe_dsp_last_error())
    assert fn(None, L.FMT_F32) == L.SFE_EINVAL and lib.sfe_dsp_last_error() == text
    assert fn(h._h, other) == L.SFE_OK and fn(h._h, L.FMT_F32) == L.SFE_OK
    h.close()
