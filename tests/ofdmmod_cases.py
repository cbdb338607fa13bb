"""The shapes, inputs and references the OFDM-modulator tests share (tests/test_ofdmmod_host.py, tests/test_gpu_ofdmmod.py):
the receiver's own shapes (tests/ofdm_cases.py) fed to the transmit side, and the float64 np.fft synthesiser
(synth.ofdm_signal) as the independent reference.  Host only: numpy and simplefe_amd.synth; nothing here touches the
library or a GPU."""
import numpy as np

import ofdm_cases as oc
from simplefe_amd import synth

BITS, SYMBOLS = 0, 1            # lib.OFDMMOD_IN_*
F32, TX10 = 0, 2                # lib.FMT_*
# the bar the project holds the receiver's float32 transforms to against float64: relative RMS error of a symbol
RMS_BAR = 1e-5
# every kernel size with every bin used, DC and N / 2 included (with and without pilots, Nd = 1 among them), and the two ends
# of the receiver's own shapes
HOST_NAMES = oc.GRID_NAMES + ["n64", "n4096"]
MODES = [("bpsk", 2, BITS), ("qpsk", 4, BITS), ("symbols", 4, SYMBOLS)]
MODE_IDS = [m[0] for m in MODES]


def shape_args(name, amp=1.0, order=4, in_mode=BITS, out_fmt=F32, cp=None, n_data=None):
    """The keyword arguments of api.ofdmmod_plan / api.OfdmMod for a receiver shape.  cp, n_data: instead of the shape's."""
    a = oc.shape_args(name)
    for k in ("advance", "cfo_mode", "cfo_skip", "out_mode", "min_gate"):
        a.pop(k)
    if cp is not None:
        a["cp"] = int(cp)
    if n_data is not None:
        a["n_data"] = int(n_data)
        if a["pilot_sign"] is not None:
            a["pilot_sign"] = np.resize(a["pilot_sign"], int(n_data))
    a.update(amp=amp, order=order, in_mode=in_mode, out_fmt=out_fmt)
    return a


def sizes(args):
    """(Nd, symbols of a frame, L = N + cp, F, what a burst reads: bytes or cf32)."""
    Nd = int(np.count_nonzero(np.asarray(args["kind"]) == 1))
    nsym, L = args["n_train"] + args["n_data"], args["n_fft"] + args["cp"]
    n = args["n_data"] * Nd
    return Nd, nsym, L, nsym * L, n if args["in_mode"] == SYMBOLS else (n * (2 if args["order"] == 4 else 1) + 7) // 8


def rows(args, n_bursts, seed, pad=0):
    """(n_bursts, what a burst reads + pad) input rows: random bytes, or random complex64 symbols of about unit size."""
    n = sizes(args)[4] + pad
    rng = np.random.default_rng(synth.SEED + seed)
    if args["in_mode"] == SYMBOLS:
        return (rng.standard_normal((n_bursts, n)) + 1j * rng.standard_normal((n_bursts, n))).astype(np.complex64) * np.float32(0.7)
    return rng.integers(0, 256, size=(n_bursts, n), dtype=np.uint8)


def sent_symbols(args, row):
    """The (Ns, Nd) data symbols of one burst as the law forms them in float32 (amp included), complex64."""
    Nd, _, _, _, n = sizes(args)
    if args["in_mode"] == SYMBOLS:
        s = np.asarray(row, np.complex64)[:n]
        out = np.empty(n, np.complex64)
        out.real, out.imag = s.real * np.float32(args["amp"]), s.imag * np.float32(args["amp"])
        return out.reshape(-1, Nd)
    bps = 2 if args["order"] == 4 else 1
    bits = np.unpackbits(np.asarray(row, np.uint8))[:args["n_data"] * Nd * bps]
    return synth.mod_symbols(bits, args["order"], args["amp"]).reshape(-1, Nd)


def reference_frame(args, row):
    """One frame by synth.ofdm_signal (float64 np.fft, one tap of 1, no offset, no noise): it has no amp, so it is handed
    amp train, amp pilot and amp-scaled symbols, each formed in float32 as the law forms them."""
    amp = np.float32(args["amp"])
    F = sizes(args)[3]

    def scaled(t):
        if t is None:
            return None
        t = np.asarray(t, np.complex64)
        out = np.empty(t.size, np.complex64)
        out.real, out.imag = amp * t.real, amp * t.imag
        return out

    return synth.ofdm_signal(args["n_fft"], args["cp"], args["n_train"], args["kind"], scaled(args["train"]), F, 0, symbols=sent_symbols(args, row),
                             pilot=scaled(args["pilot"]), pilot_sign=args["pilot_sign"])


def worst_symbol_rms(got_frame, want_frame, args):
    """The largest relative RMS error of a symbol of the frame."""
    _, nsym, L, _, _ = sizes(args)
    g, w = np.asarray(got_frame).reshape(nsym, L), np.asarray(want_frame).reshape(nsym, L)
    return max(oc.rel_rms(g[j], w[j]) for j in range(nsym))


def exact_args(name, out_fmt=F32):
    """The exact case on a shape's sizes: every bin a data bin, order 2, amp 1, train all ones, no pilots, T = 1."""
    sh = oc.shape(name)
    N = sh["n_fft"]
    return dict(n_fft=N, cp=sh["cp"], n_train=1, n_data=sh["n_data"], kind=np.ones(N, np.uint8), train=np.ones(N, np.complex64), pilot=None,
                pilot_sign=None, amp=1.0, order=2, in_mode=BITS, out_fmt=out_fmt)


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))
