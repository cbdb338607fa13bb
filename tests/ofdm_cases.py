"""The shapes, channels and waveforms the OFDM-receiver tests share (tests/test_ofdm_host.py, tests/test_gpu_ofdm.py,
tests/test_gpu_ofdm_grid.py).
Host only: numpy and simplefe_amd.synth; nothing here touches the library or a GPU."""
import numpy as np

from simplefe_amd import synth

# name: the shape (the arguments of sfe_dsp_ofdm_create), the bins, the FIR channel as {delay: tap} and the frequency offset
# in subcarrier spacings.  The channels have 2 or 3 taps; where there is a guard (cp - advance > 0) they end inside it.  Two
# shapes have none: n128 has no prefix at all, n512 starts its window at the prefix's first sample, so the second tap of
# their channels leaks one sample of the symbol before into the window -- a floor under their error vectors, counted in WORST.
SHAPES = {
    # 54 data bins and 4 pilots; even log2 N; the chain's shape
    "n64": dict(n_fft=64, cp=16, advance=4, n_train=2, n_data=6, cfo_mode=1, cfo_skip=6, used=29, pilots=(7, 21),
                taps={0: 1.0, 2: 0.45 * np.exp(0.7j), 5: 0.25 * np.exp(-1.9j)}, eps=0.13),
    # cfo_mode 0; odd log2 N; no prefix; one training and one data symbol
    "n128": dict(n_fft=128, cp=0, advance=0, n_train=1, n_data=1, cfo_mode=0, cfo_skip=0, used=50, pilots=(10, 30, 45),
                 taps={0: 0.9 * np.exp(0.4j), 1: 0.1 * np.exp(2.2j)}, eps=0.0),
    # cp = N, advance = cp, four training symbols; 300 data bins (no multiple of 64); no pilots
    "n512": dict(n_fft=512, cp=512, advance=512, n_train=4, n_data=3, cfo_mode=1, cfo_skip=8, used=150, pilots=(),
                 taps={0: 1.1 * np.exp(-0.3j), 1: 0.12 * np.exp(1.3j)}, eps=-0.13),
    # the LDS limit; half the prefix skipped by the offset estimator; 3000 data bins and 200 pilots
    "n4096": dict(n_fft=4096, cp=288, advance=0, n_train=1, n_data=2, cfo_mode=1, cfo_skip=144, used=1600, pilots=tuple(range(8, 1600, 16)),
                  taps={0: 1.0, 3: 0.4 * np.exp(2.5j), 11: 0.2 * np.exp(-0.8j)}, eps=-0.31),
}
NAMES = list(SHAPES)

# One shape per kernel size, log2 N = 6 .. 12, with EVERY bin used -- DC and N / 2 included -- so that the whole of every
# transform's output is compared: data_k None is "all bins that are no pilot", pilot_k the pilot bins themselves.  The window
# starts four samples before the prefix ends and the 3-tap channel, its first tap dominant, ends inside those four.  Between
# them: T = 1 .. 4; cfo_skip = 0 and cp - 1 (one product per symbol); cp odd and smaller than the workgroup, N + cp no
# multiple of it; cfo_mode 0; no pilots, one, two, and more pilots than lanes; and one data bin alone (Nd = 1, bin N - 1).
def _grid(n_fft, cp, advance, n_train, n_data, spacing, cfo_skip, eps, cfo_mode=1, data_k=None, turn=0.0):
    pilot_k = () if spacing is None else tuple(range(spacing // 2, n_fft, spacing))
    return dict(n_fft=n_fft, cp=cp, advance=advance, n_train=n_train, n_data=n_data, cfo_mode=cfo_mode, cfo_skip=cfo_skip, data_k=data_k,
                pilot_k=pilot_k, taps={0: np.exp(1j * turn), 1: 0.3 * np.exp(1j * (1.0 + turn)), 3: 0.15 * np.exp(1j * (turn - 2.0))}, eps=eps)


GRID = {
    "g64": _grid(64, 16, 12, 2, 3, 8, 15, 0.21),                        # 8 pilots; cfo_skip = cp - 1
    "g128": _grid(128, 9, 5, 4, 2, 16, 0, -0.08, turn=0.5),             # T = 4; cp odd, below the 64 lanes
    "g256": _grid(256, 7, 3, 3, 2, 16, 6, 0.33, turn=-1.1),             # T = 3; four butterflies per lane in one wave
    "g512": _grid(512, 40, 36, 1, 2, None, 0, -0.27, turn=2.0),         # no pilots
    "g1024": _grid(1024, 100, 96, 2, 2, 64, 99, 0.11, turn=0.9),        # four waves; cfo_skip = cp - 1
    "g2048": _grid(2048, 33, 29, 1, 1, 1024, 32, -0.19, turn=-0.4),     # two pilots; a radix-2 pass before multi-element radix-4 passes
    "g4096": _grid(4096, 24, 20, 1, 1, 3, 0, 0.0, cfo_mode=0, turn=1.7),            # 1366 pilots on 256 lanes; cfo_mode 0
    "g2048one": _grid(2048, 33, 29, 2, 3, None, 0, 0.26, data_k=(2047,), turn=0.3),            # Nd = 1, no pilots
    "g128p1": _grid(128, 9, 5, 1, 2, 128, 8, 0.45, turn=-2.3),          # Np = 1: the one pilot is bin N / 2; eps near the half
}
GRID_NAMES = list(GRID)

# The long burst: the n64 shape's bins, pilots and channel with 1024 data symbols -- 82 080 samples, and with eps near a half
# the turn count eps n / N passes 500: formed in float32 it is rounded to some 3e-5 of a turn before it is reduced, formed in
# float64 and reduced first, as the law says, to 1e-13.
LONG = {name: dict(SHAPES["n64"], n_data=1024, eps=eps) for name, eps in (("long+", 0.4), ("long-", -0.47))}
LONG_NAMES = list(LONG)


def shape(name):
    return SHAPES[name] if name in SHAPES else GRID[name] if name in GRID else LONG[name]


def bursts(name):
    """Bursts in a shape's stream: three, one of the long burst."""
    return 1 if name in LONG else 3
RATIO_BAR = 1.0 / 16.0          # min_used |H|^2 / h2 of every equalised case

# The worst error vector |Z - sent| of the float64 plan over each shape's noiseless bursts (zero-forcing output), as
# tests/test_ofdm_host.py printed it; later runs are held to twice it.
WORST = {"n64": 1.885e-7, "n128": 1.898e-2, "n512": 1.027e-2, "n4096": 2.149e-7}


def tables(name):
    """kind uint8 [N], train complex64 [N], pilot complex64 [N] or None, pilot_sign int8 [Ns] or None."""
    sh = shape(name)
    N, Ns = sh["n_fft"], sh["n_data"]
    k = np.arange(N)
    f = np.where(k < N // 2, k, k - N)                  # the bin's signed frequency
    if "pilot_k" in sh:                                 # a GRID shape: the bins themselves
        kind = np.ones(N, np.uint8) if sh["data_k"] is None else np.isin(k, sh["data_k"]).astype(np.uint8)
        kind[list(sh["pilot_k"])] = 2
    else:
        kind = np.where((np.abs(f) <= sh["used"]) & (f != 0), 1, 0).astype(np.uint8)
        kind[np.isin(np.abs(f), sh["pilots"])] = 2
    has_pilots = bool((kind == 2).any())
    seed = synth.SEED + N
    train = (synth.psk_symbols(N, 4, seed=seed) * (1.0 + 0.25 * np.cos(0.37 * k))).astype(np.complex64)
    if not has_pilots:
        return kind, train, None, None
    pilot = (synth.psk_symbols(N, 2, seed=seed + 1) * 1.25).astype(np.complex64)
    sign = np.where(synth.vit_bits(Ns, seed=seed + 2) == 1, -1, 1).astype(np.int8)
    return kind, train, pilot, sign


def shape_args(name, out_mode=0, min_gate=0.0):
    """The keyword arguments of api.ofdm_plan / api.Ofdm for a shape."""
    sh = shape(name)
    kind, train, pilot, sign = tables(name)
    return dict(n_fft=sh["n_fft"], cp=sh["cp"], advance=sh["advance"], n_train=sh["n_train"], n_data=sh["n_data"], kind=kind, train=train,
                pilot=pilot, pilot_sign=sign, cfo_mode=sh["cfo_mode"], cfo_skip=sh["cfo_skip"], out_mode=out_mode, min_gate=min_gate)


def reference_args(name, out_mode=0):
    a = shape_args(name, out_mode)
    a.pop("min_gate")
    return a


def reach(name):
    sh = shape(name)
    return (sh["n_train"] + sh["n_data"]) * (sh["n_fft"] + sh["cp"])


def n_data_bins(name):
    return int(np.count_nonzero(tables(name)[0] == 1))


def channel(name):
    taps = shape(name)["taps"]
    h = np.zeros(max(taps) + 1, np.complex128)
    for d, v in taps.items():
        h[d] = v
    return h


def sent_symbols(name, b, seed=0):
    """The (n_data, Nd) unit QPSK symbols burst b carries, complex64."""
    sh = shape(name)
    Nd = n_data_bins(name)
    bits = synth.vit_bits(2 * sh["n_data"] * Nd, seed=synth.SEED + 1000 * seed + 17 * b + sh["n_fft"])
    return synth.mod_symbols(bits, 4, 1.0).reshape(sh["n_data"], Nd)


_streams = {}


def stream(name, n_bursts=None, noise=0.0, gain=1.0, seed=0):
    """One stream of n_bursts bursts of a shape through its channel and offset: (x complex64, starts int64 [n_bursts], the
    sent symbols (n_bursts, n_data, Nd)).  Burst b starts 11 + 3 b samples into its slot of reach + 40 samples.  Cached:
    callers must not write into what they get."""
    n_bursts = bursts(name) if n_bursts is None else n_bursts
    key = (name, n_bursts, noise, gain, seed)
    if key not in _streams:
        sh = shape(name)
        kind, train, pilot, sign = tables(name)
        slot = reach(name) + 40
        starts = np.array([b * slot + 11 + 3 * b for b in range(n_bursts)], np.int64)
        sent = np.stack([sent_symbols(name, b, seed) for b in range(n_bursts)])
        x = np.zeros(n_bursts * slot, np.complex128)
        for b in range(n_bursts):
            x += synth.ofdm_signal(sh["n_fft"], sh["cp"], sh["n_train"], kind, train, x.size, starts[b], symbols=sent[b], pilot=pilot,
                                   pilot_sign=sign, taps=channel(name), eps=sh["eps"])
        if noise:
            rng = np.random.default_rng(synth.SEED + seed)
            x = x + noise * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
        x = (gain * x).astype(np.complex64)
        x.setflags(write=False)
        _streams[key] = (x, starts, sent)
    return _streams[key]


_refs = {}


def reference(name, out_mode=0, n_bursts=None):
    """synth.ofdm_reference over stream(name, n_bursts): (symbols (n_bursts, n_data, Nd), chan (n_bursts, N), record
    (n_bursts, 8), status (n_bursts,)).  Cached."""
    n_bursts = bursts(name) if n_bursts is None else n_bursts
    key = (name, out_mode, n_bursts)
    if key not in _refs:
        x, starts, _ = stream(name, n_bursts)
        rows = [synth.ofdm_reference(x, int(o), **reference_args(name, out_mode)) for o in starts]
        _refs[key] = tuple(np.stack([np.asarray(r[i]) for r in rows]) for i in range(4))
    return _refs[key]


def exact_case(name, n_bursts=2):
    """The exact case on a shape's sizes: cfo_mode 0, no pilots, T = 1, train all ones, and x = 1+0j at every window's first
    sample and +0 elsewhere: (keyword arguments without out_mode, x, starts)."""
    sh = shape(name)
    N, cp, g, Ns = sh["n_fft"], sh["cp"], sh["advance"], sh["n_data"]
    kind = (tables(name)[0] != 0).astype(np.uint8)
    args = dict(n_fft=N, cp=cp, advance=g, n_train=1, n_data=Ns, kind=kind, train=np.ones(N, np.complex64), pilot=None, pilot_sign=None,
                cfo_mode=0, cfo_skip=0)
    L, R = N + cp, (1 + Ns) * (N + cp)
    starts = np.array([5 + b * (R + 3) for b in range(n_bursts)], np.int64)
    x = np.zeros(n_bursts * (R + 3) + 8, np.complex64)
    for o in starts:
        x[o + np.arange(1 + Ns) * L + cp - g] = 1.0
    return args, x, starts


def rel_rms(got, want):
    want = np.asarray(want, np.complex128)
    return float(np.sqrt((np.abs(np.asarray(got, np.complex128) - want) ** 2).sum() / (np.abs(want) ** 2).sum()))


# the condition on the inputs: every equalised case keeps its weakest used bin within 12 dB of the mean
for _name in NAMES + GRID_NAMES + LONG_NAMES:
    _rec, _st = reference(_name)[2:]
    assert not _st.any() and (_rec[:, 2] >= RATIO_BAR).all(), (_name, _rec[:, 2])


# ---- the chain Ldpc.encode_stream -> (host: ofdm_signal) -> Corr -> Ofdm (MRC) -> Ldpc.process_stream on the n64 shape:
# code B of tests/ldpc_cases.py, n = 648 = 2 * 6 * 54.  Three bursts in blocks 1, 2 and 3 of five correlator blocks (the receiver is
# pointed at the three: every status of the chain is 0); a
# 3-tap channel with a dominant first tap; eps = 0.1.  CHAIN_NOISE and CHAIN_SEED were chosen on the CPU through the host
# plans (chain_on_the_cpu checks what they were chosen for): the correlator's peaks stand where the bursts start, ahead of
# the second training symbol's equal-looking peak by CHAIN_MARGIN at least, one burst or more reaches the decoder with
# wrong hard decisions, and every codeword converges to its payload.
CHAIN = dict(block=3840, n_blocks=5, at={1: 3840 + 500, 2: 2 * 3840 + 1717, 3: 3 * 3840 + 100}, eps=0.1, min_gate=0.5,
             taps={0: 1.0, 1: 0.3 * np.exp(1.0j), 3: 0.15 * np.exp(-2.0j)})
CHAIN_NOISE, CHAIN_SEED, CHAIN_MARGIN = 0.04, 4, 0.01


def chain_signal(code_bits, noise=None, seed=None):
    """The chain's stream, complex64: code_bits (3, 648) uint8, one codeword per burst."""
    sh, c = SHAPES["n64"], CHAIN
    kind, train, pilot, sign = tables("n64")
    n = c["n_blocks"] * c["block"]
    h = np.zeros(max(c["taps"]) + 1, np.complex128)
    for d, v in c["taps"].items():
        h[d] = v
    x = np.zeros(n, np.complex128)
    for bits, o in zip(code_bits, c["at"].values()):
        x += synth.ofdm_signal(64, 16, 2, kind, train, n, o, bits=bits, pilot=pilot, pilot_sign=sign, taps=h, eps=c["eps"])
    rng = np.random.default_rng(synth.SEED + 4242 + (CHAIN_SEED if seed is None else seed))
    s = CHAIN_NOISE if noise is None else noise
    return (x + s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def chain_template():
    """The correlator's one template: the first training symbol's waveform as sent, prefix included (80 samples)."""
    kind, train, pilot, sign = tables("n64")
    return synth.ofdm_signal(64, 16, 1, kind, train, 80, 0, symbols=np.zeros((0, n_data_bins("n64"))))


def chain_on_the_cpu(api, L, lc, noise=None, seed=None):
    """The chain through the host plans: (x, payloads (3, 41), the correlator reference's (peak_val, peak_idx) per block,
    ldpc_plan's (bytes, record, status) behind ofdm_plan's MRC symbols, ofdm_plan's records (3, 8)).  Asserts what the noise was chosen for."""
    c = CHAIN
    s, Z = lc.CASES["B"]
    a_, beta, max_iter = lc.PARAMS["a12"]
    pay = lc.payloads("B", 3, 77)
    code = np.unpackbits(api.ldpc_plan(s, Z, data=pay), axis=1)[:, :648]
    x = chain_signal(code, noise, seed)
    tpl = chain_template()
    m, val, idx = synth.corr_reference(x, tpl[None, :], c["block"], 0.0)
    for j, o in c["at"].items():
        assert idx[0, j] == o - j * c["block"] + 79, (j, idx[0, j])
        assert m[0, o + 79] >= (1.0 + CHAIN_MARGIN) * m[0, o + 159] and val[0, j] >= 1.2 * c["min_gate"]
    assert (val[0, [0, 4]] <= 0.8 * c["min_gate"]).all()
    sym, ch, rec, st = api.ofdm_plan(x=x, idx=idx[0, 1:4].astype(np.uint32), gate=val[0, 1:4].astype(np.float32), start_base=c["block"] - 79,
                                     start_step=c["block"], **shape_args("n64", 1, c["min_gate"]))
    assert not st.any()
    dec = api.ldpc_plan(s, Z, lc.SCALE, a_, beta, max_iter, in_mode=L.VIT_IN_QPSK, skip=0, x=sym.reshape(3, -1), status_in=st)
    assert not dec[2].any() and np.array_equal(dec[0], lc.payload_bits_only("B", pay))
    assert dec[1][:, 2].max() >= 1                      # decisions that left the input's sign: repairs
    return x, pay, (val[0], idx[0]), dec, rec
