"""What tests/test_reed_host.py and tests/test_gpu_reed.py share: the shapes of the Reed-Solomon outer code, the error patterns
laid over encoded frames, the reference's verdict on them (computed once per shape and left unchanged), and the small link
of the chain test.  Frames are built with synth.reed_reference alone; nothing here calls the library."""
import functools

import numpy as np

import mod_checks as mc
from simplefe_amd import synth

# (prim, fcr, step, n, n_par, depth)
SHAPES = {
    "A": (0x187, 112, 11, 255, 32, 4),      # the frame vit can carry: 1020 bytes
    "B": (0x11d, 0, 1, 255, 64, 1),         # every lane holds a syndrome
    "C": (0x11d, 1, 1, 40, 8, 3),           # shortened
    "D": (0x11d, 0, 1, 3, 2, 16),           # k = 1, t = 1, the deepest interleave
    "E": (0x187, 112, 11, 65, 5, 2),        # odd n_par, one position past a wave
    "F": (0x11d, 254, 254, 255, 2, 1),      # the edges of fcr and step
}
# seeds of the t + 1 patterns: under the reference alone they hold an uncorrectable codeword on A, B, C and E and a
# miscorrection on F (asserted by the tests before anything is compared)
SEEDS = {"A": 101, "B": 102, "C": 103, "D": 104, "E": 105, "F": 106}


def sizes(shape):
    prim, fcr, step, n, n_par, I = shape
    return I * (n - n_par), I * n, n_par // 2


def whitening(shape, seed=7):
    return np.random.default_rng(seed).integers(0, 256, size=sizes(shape)[1], dtype=np.uint8)


def payloads(shape, n_frames, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(int(n_frames), sizes(shape)[0]), dtype=np.uint8)


def hit(frame, I, i, places, rng):
    """Codeword i of the frame gets a wrong byte (a nonzero difference) at each of its byte positions `places`."""
    for j in places:
        frame[j * I + i] ^= np.uint8(rng.integers(1, 256))


def padded_word(shape, p, v=1):
    """The n bytes of the word whose message is zero and whose parity is v x^p mod g(x), p >= n: the full-length codeword
    v x^p + (v x^p mod g) differs from it in the padded position p alone."""
    prim, fcr, step, n, n_par, I = shape
    assert p >= n
    _, _, g = synth.reed_tables(prim, fcr, step, n, n_par)
    full = np.zeros((1, p + 1 - n_par), np.uint32)
    full[0, 0] = v                                      # v x^p as a message of p + 1 - n_par bytes: byte 0 is x^p
    parity = synth.reed_encode_words(full, g, prim)[0, -n_par:]
    return np.concatenate([np.zeros(n - n_par, np.uint8), parity.astype(np.uint8)])


@functools.lru_cache(maxsize=None)
def patterns(key, with_whitening=True):
    """(names, payloads (F, P), channel frames (F, Fb), whitening or None): a frame per pattern (three for `ends`), every
    codeword of a frame hit by its pattern at places of its own."""
    shape = SHAPES[key]
    prim, fcr, step, n, n_par, I = shape
    P, Fb, t = sizes(shape)
    k = n - n_par
    rng = np.random.default_rng(SEEDS[key])
    wh = whitening(shape) if with_whitening else None
    names, pay, frames = [], [], []

    def fresh(name):
        names.append(name)
        pay.append(payloads(shape, 1, 1000 + len(names))[0])
        frames.append(synth.reed_reference(*shape, pay[-1], whiten=wh, encode=True)[0].copy())
        return frames[-1]

    fresh("clean")
    for e in (1, t, t + 1, n):
        f = fresh("%d wrong" % e if e not in (t + 1,) else "t+1 wrong")
        for i in range(I):
            hit(f, I, i, rng.choice(n, size=min(e, n), replace=False), rng)
    f = fresh("parity only")
    for i in range(I):
        hit(f, I, i, k + rng.choice(n_par, size=t, replace=False), rng)
    for name, places in (("byte 0", [0]), ("byte n-1", [n - 1])) + ((("both ends", [0, n - 1]),) if t >= 2 else ()):
        f = fresh(name)
        for i in range(I):
            hit(f, I, i, places, rng)
    for name, run in (("run I t", I * t), ("run I t + 1", I * t + 1)):
        f = fresh(name)
        at = int(rng.integers(0, Fb - run + 1))
        f[at:at + run] ^= rng.integers(1, 256, size=run, dtype=np.uint8)
    if key in ("C", "E"):
        names.append("padded position")
        pay.append(np.zeros(P, np.uint8))
        words = np.stack([padded_word(shape, n + 3 * i, v=1 + i) for i in range(I)])        # codeword i: p = n + 3 i
        frames.append(np.ascontiguousarray(words.T).reshape(-1) ^ (wh if wh is not None else 0))
    return tuple(names), np.stack(pay), np.stack(frames).astype(np.uint8), wh


@functools.lru_cache(maxsize=None)
def reference(key, with_whitening=True):
    """(bytes, record, status) of the patterns' frames under synth.reed_reference."""
    names, pay, frames, wh = patterns(key, with_whitening)
    return synth.reed_reference(*SHAPES[key], frames, whiten=wh)


def check_the_reference(key):
    """What the law must give on the patterns, asserted on the reference alone: within t everything comes back; the t + 1
    frame holds an uncorrectable codeword (A, B, C, E) or a miscorrection (F); the padded word is uncorrectable."""
    names, pay, frames, wh = patterns(key)
    by, rec, st = reference(key)
    prim, fcr, step, n, n_par, I = SHAPES[key]
    P, Fb, t = sizes(SHAPES[key])
    for f, name in enumerate(names):
        if name in ("clean", "1 wrong", "%d wrong" % t, "parity only", "byte 0", "byte n-1", "both ends", "run I t"):
            assert st[f] == 0 and np.array_equal(by[f], pay[f]), (key, name)
        if name == "clean":
            assert rec[f].tolist() == [0, 0]
        if name in ("1 wrong", "byte 0", "byte n-1"):
            assert rec[f].tolist() == [I, 0], (key, name)
        if name in ("%d wrong" % t, "parity only"):
            assert rec[f].tolist() == [I * t, 0], (key, name)
        if name == "run I t":
            assert rec[f].tolist() == [I * t, 0], (key, name)
        if name == "t+1 wrong" and key in "ABCE":
            assert st[f] == 1 and rec[f, 1] != 0, (key, name)
        if name == "t+1 wrong" and key == "F":
            assert st[f] == 0 and not np.array_equal(by[f], pay[f]), (key, name)
        if name == "padded position":
            assert st[f] == 1 and rec[f].tolist() == [0, (1 << I) - 1] and not by[f].any(), (key, name)


def many(key, n_frames):
    """(channel frames (n_frames, Fb), whitening): the patterns' frames, repeated in their order up to n_frames."""
    names, pay, frames, wh = patterns(key)
    idx = np.arange(int(n_frames)) % frames.shape[0]
    return np.ascontiguousarray(frames[idx]), wh


# ---- the chain Reed.encode_stream -> Mod -> Corr -> Burst -> Vit -> Reed.process_stream: the loopback of mod_checks with a
# shortened outer code in front of it and behind it
LINK_CODE = (0x11d, 1, 1, 20, 8, 2)         # P = 24, Fb = 40, t = 4: n_info = 320
LINK = dict(mc.CHAIN, n_info=320, N=32 + 2 * (320 + 6), F=(32 + 2 * (320 + 6) + 16) * 10, step=7168, n_bursts=3)


def link_parts():
    """(taps, preamble, the correlator's template) of mod_checks' loopback, the payloads (3, 24), the whitening (40,)."""
    taps, pre, _, tpl = mc.chain_parts()
    return taps, pre, tpl, payloads(LINK_CODE, LINK["n_bursts"], 77), whitening(LINK_CODE, 78)


def link_on_the_cpu(api, L):
    """The link through the host plans, frame 1's waveform negated over a stretch of data symbols chosen so that the inner
    decoder's bytes for that frame are wrong and no codeword of the outer code holds more than t of them.  Returns (the
    stretch's first and last + 1 sample, the encoded frames, vit_plan's bytes, reed_plan's (bytes, record, status))."""
    c = LINK
    taps, pre, tpl, pay, wh = link_parts()
    frames = api.reed_plan(*LINK_CODE, whiten=wh, data=pay, encode=True)
    x = api.mod_plan(c["K"], c["gen"], c["n_info"], taps, c["sps"], preamble=pre, amp=c["amp"], data=frames, n_out=c["n_bursts"] * c["step"],
                     start_base=c["base"], start_step=c["step"])
    peak0 = c["base"] + c["tpl_at"]                     # symbol 0's peak in frame 0
    for n_sym in (24, 32, 40, 48, 56, 64):
        a = peak0 + c["step"] + c["sps"] * (c["Lp"] + 200) - c["sps"] // 2
        b = a + c["sps"] * n_sym
        y = x.copy()
        y[a:b] = -y[a:b]
        sym = api.burst_plan(pre, c["sps"], c["N"], c["lag"], x=y, n_bursts=c["n_bursts"], start_base=peak0, start_step=c["step"])[0]
        by = api.vit_plan(c["K"], c["gen"], c["n_info"], in_mode=L.VIT_IN_BPSK, skip=c["Lp"], x=sym)[0]
        dec = api.reed_plan(*LINK_CODE, whiten=wh, data=by)
        if not np.array_equal(by[1], frames[1]) and not dec[2].any():
            return (a, b), frames, by, dec
    raise AssertionError("no stretch damages the inner decoder's bytes within the outer code's reach")
