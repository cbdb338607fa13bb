"""What tests/test_ldpc_host.py and tests/test_gpu_ldpc.py share: the test codes of the quasi-cyclic LDPC block
(sfe_dsp_ldpc_*), built here from seeds and from nothing else, their inputs, and synth.ldpc_reference's answers, computed once.

qc(mb, nb, Z, seed, wcol): information columns get `wcol` distinct rows with uniform shifts; the parity part is the
dual-diagonal form of 802.11n / 802.16e -- its first column has shift 1 mod Z in rows 0 and mb - 1 and shift 0 in row
mb // 2, column j >= 1 has shift 0 in rows j - 1 and j -- which is invertible by construction.

Inputs per case: seeded payloads encoded by the reference, BPSK of unit amplitude (+1 is bit 0) plus Gaussian noise in three
groups -- clean; noisy at EBN0[key], at which the reference converges on every word of the group for both parameter sets
(searched on the CPU in steps of half a dB from the rate's rule of thumb, then fixed here); hopeless at -2 dB -- and the
special words: +0, -0, +-3e38 (the product overflows and clamps), rounding ties (x.5 / scale), one NaN and one inf word."""
import functools

import numpy as np

import mod_checks as mc
from simplefe_amd import synth

F32 = np.float32
SCALE = 8.0
PARAMS = {"a12": (12, 0, 32), "a16": (16, 1, 5)}       # (a, beta, max_iter)
N_CLEAN, N_NOISY, N_HOPELESS = 2, 6, 3
HOPELESS_DB = -2.0


def qc(mb, nb, Z, seed, wcol):
    rng = np.random.default_rng(seed)
    s = np.full((mb, nb), -1, np.int16)
    kb = nb - mb
    for c in range(kb):
        rows = rng.choice(mb, size=wcol, replace=False)
        s[rows, c] = rng.integers(0, Z, size=wcol)
    s[0, kb] = s[mb - 1, kb] = 1 % Z
    s[mb // 2, kb] = 0
    for j in range(1, mb):
        s[j - 1, kb + j] = s[j, kb + j] = 0
    return s


def hamming():
    """Hamming (7, 4) as a 3 x 7 base matrix with Z = 1: H = [A | I]."""
    A = np.array([[1, 1, 0, 1], [1, 0, 1, 1], [0, 1, 1, 1]])
    return np.where(np.concatenate([A, np.eye(3, dtype=int)], axis=1) == 1, 0, -1).astype(np.int16)


def _not_encodable():
    s = qc(3, 6, 7, 101, 2).copy()
    s[:, 5] = s[:, 4]
    return s


# key -> (base matrix, Z)
CASES = {
    "H": (hamming(), 1),
    "A": (qc(3, 6, 7, 101, 2), 7),                  # Z far below a wave
    "B": (qc(12, 24, 27, 102, 3), 27),              # Z neither a multiple of 4 nor of the wave
    "C": (qc(12, 24, 64, 103, 3), 64),              # Z exactly a wave
    "D": (qc(4, 33, 32, 104, 4), 32),               # a block row of exactly 32 cells, rate 29/33
    "E": (qc(12, 24, 341, 105, 3), 341),            # Z above a workgroup's thread count, odd, k not a whole byte count
    "F": (qc(8, 16, 512, 106, 3), 512),             # n and Z both at their limits
    "G": (_not_encodable(), 7),                     # A with its last parity column a copy of the one before: not encodable
}
ENCODABLE = [k for k in sorted(CASES) if k != "G"]
# Eb/N0 in dB of the noisy group (G has no codewords of its own: its inputs are A's words)
EBN0 = {"H": 9.0, "A": 8.0, "B": 4.0, "C": 3.5, "D": 6.0, "E": 3.5, "F": 3.5, "G": 8.0}


def sizes(key):
    """(n, k, k_bytes, n_bytes)."""
    s, Z = CASES[key]
    n, k = s.shape[1] * Z, (s.shape[1] - s.shape[0]) * Z
    return n, k, (k + 7) // 8, (n + 7) // 8


def payloads(key, n_words, seed):
    """(n_words, k_bytes) random bytes: the pad bits of the last byte are random too (the law ignores them)."""
    return np.random.default_rng(seed).integers(0, 256, size=(int(n_words), sizes(key)[2]), dtype=np.uint8)


def payload_bits_only(key, pay):
    """The payload bytes with their pad bits cleared: what a decoder writes."""
    n, k, kb, nb = sizes(key)
    out = pay.copy()
    if k & 7:
        out[:, -1] &= (0xFF00 >> (k & 7)) & 0xFF
    return out


@functools.lru_cache(maxsize=None)
def words(key):
    """(payloads with pad bits cleared, the reference's codeword bits (W, n) uint8) for the case's W words; G borrows A's
    codewords: they are not codewords of G, which is the point of a code that cannot be encoded."""
    src = "A" if key == "G" else key
    n, k, kb, nb = sizes(src)
    W = N_CLEAN + N_NOISY + N_HOPELESS + 4
    pay = payloads(src, W, 1000 + ord(src))
    code = synth.ldpc_encode_reference(*CASES[src], pay)
    return payload_bits_only(src, pay), np.unpackbits(code, axis=1)[:, :n]


def sigma(key, db):
    n, k, kb, nb = sizes(key)
    return float(np.sqrt(1.0 / (2.0 * (k / n) * 10.0 ** (db / 10.0))))


@functools.lru_cache(maxsize=None)
def inputs(key):
    """(names, x (W, n) float32): a name per row -- "clean", "noisy", "hopeless" or a special word's."""
    n, k, kb, nb = sizes(key)
    pay, bits = words(key)
    tx = (1.0 - 2.0 * bits).astype(np.float64)
    rng = np.random.default_rng(2000 + ord(key))
    names, rows, w = [], [], 0
    for name, count, sd in (("clean", N_CLEAN, 0.0), ("noisy", N_NOISY, sigma(key, EBN0[key])), ("hopeless", N_HOPELESS, sigma(key, HOPELESS_DB))):
        for _ in range(count):
            rows.append(tx[w] + sd * rng.standard_normal(n))
            names.append(name)
            w += 1
    rows.append(np.zeros(n)), names.append("+0")
    rows.append(-np.zeros(n)), names.append("-0")
    rows.append(3e38 * tx[w]), names.append("3e38")
    rows.append(tx[w + 1] * ((np.arange(n) % 20) + 0.5) / SCALE), names.append("ties")
    bad = tx[w + 2].copy()
    bad[n // 2] = np.nan
    rows.append(bad), names.append("nan")
    bad = tx[w + 3].copy()
    bad[n - 1] = -np.inf
    rows.append(bad), names.append("inf")
    return tuple(names), np.stack(rows).astype(F32)


def word_of(key, name):
    """The index into words(key) of the row called `name` (the groups and "3e38", "ties")."""
    base = N_CLEAN + N_NOISY + N_HOPELESS
    return {"3e38": base, "ties": base + 1}.get(name)


@functools.lru_cache(maxsize=None)
def reference(key, pset):
    """(bytes, record, status, peak |APP|) of inputs(key) under synth.ldpc_reference with PARAMS[pset]."""
    a, beta, max_iter = PARAMS[pset]
    return synth.ldpc_reference(*CASES[key], inputs(key)[1], scale=SCALE, a=a, beta=beta, max_iter=max_iter, with_peak=True)


def check_the_reference(key, pset):
    """What the law must give on the inputs, asserted on the reference alone."""
    names, x = inputs(key)
    by, rec, st, peak = reference(key, pset)
    pay, bits = words(key)
    own = key != "G"                # G's inputs are no codewords of G: only the reference decides what comes back
    for i, name in enumerate(names):
        if name == "clean" and own:
            assert st[i] == 0 and rec[i].tolist() == [0, 0, 0] and np.array_equal(by[i], pay[i]), (key, pset, i)
        if name == "noisy" and own:
            assert st[i] == 0 and rec[i, 1] == 0 and np.array_equal(by[i], pay[i]), (key, pset, i, rec[i])
        if name in ("+0", "-0"):
            assert st[i] == 0 and rec[i].tolist() == [0, 0, 0] and not by[i].any(), (key, pset, name)
        if name == "3e38" and own:
            assert st[i] == 0 and rec[i].tolist() == [0, 0, 0] and np.array_equal(by[i], pay[word_of(key, name)]), (key, pset)
        if name in ("nan", "inf"):
            assert st[i] == 1 and not rec[i].any() and not by[i].any(), (key, pset, name)
    hopeless = [i for i, nm in enumerate(names) if nm == "hopeless"]
    assert any(st[i] == 3 and rec[i, 0] == PARAMS[pset][2] and rec[i, 1] > 0 for i in hopeless), (key, pset, st[hopeless])
    if own and key != "H":
        assert any(rec[i, 0] >= 1 for i, nm in enumerate(names) if nm == "noisy"), (key, pset)      # the group is not clean by another name


def as_mode(x, mode, skip):
    """The rows of soft values laid out for an input mode (0 soft, 1 BPSK, 2 QPSK): complex rows behind `skip` symbols.
    Every float the law does not read is a NaN."""
    x = np.asarray(x, F32)
    W, n = x.shape
    if mode == 0:
        return x
    ns = n if mode == 1 else (n + 1) // 2
    raw = np.full((W, 2 * (skip + ns)), np.nan, F32)
    if mode == 1:
        raw[:, 2 * skip::2] = x
    else:
        raw[:, 2 * skip:2 * skip + n] = x
    return raw.view(np.complex64)


def many(key, n_words):
    """inputs(key)'s rows repeated in their order up to n_words, from a rotating start so that one word is not always word 0."""
    names, x = inputs(key)
    idx = (np.arange(int(n_words)) + 3) % x.shape[0]
    return np.ascontiguousarray(x[idx])


# ---- the chain Ldpc.encode_stream -> Mod (uncoded, QPSK) -> Corr -> Burst -> Ldpc.process_stream: the loopback of mod_checks
# with case B's code in front of it and behind it
LINK_KEY = "B"
LINK = dict(mc.CHAIN, n_info=648, N=32 + 324, F=(32 + 324 + 16) * 10, step=7168, n_bursts=3)
LINK_PARAMS = PARAMS["a12"]


def link_parts():
    """(taps, preamble, the correlator's template) of mod_checks' loopback, and the payloads (3, 41)."""
    taps, pre, _, tpl = mc.chain_parts()
    return taps, pre, tpl, payloads(LINK_KEY, LINK["n_bursts"], 77)


def link_on_the_cpu(api, L):
    """The link through the host plans, burst 1's waveform negated over a stretch of data symbols chosen so that the decoder
    has wrong decisions to repair there and does repair them.  Returns (the stretch's first and last + 1 sample, the
    codewords, ldpc_plan's (bytes, record, status) behind the burst demodulator's plan)."""
    c = LINK
    s, Z = CASES[LINK_KEY]
    a_, beta, max_iter = LINK_PARAMS
    taps, pre, tpl, pay = link_parts()
    code = api.ldpc_plan(s, Z, data=pay)
    x = api.mod_plan(0, None, c["n_info"], taps, c["sps"], order=4, preamble=pre, amp=c["amp"], data=code, n_out=c["n_bursts"] * c["step"],
                     start_base=c["base"], start_step=c["step"])
    peak0 = c["base"] + c["tpl_at"]                     # symbol 0's peak in burst 0
    for n_sym in (3, 2, 4, 1, 5, 6):
        a = peak0 + c["step"] + c["sps"] * (c["Lp"] + 100) - c["sps"] // 2
        b = a + c["sps"] * n_sym
        y = x.copy()
        y[a:b] = -y[a:b]
        sym = api.burst_plan(pre, c["sps"], c["N"], c["lag"], x=y, n_bursts=c["n_bursts"], start_base=peak0, start_step=c["step"])[0]
        dec = api.ldpc_plan(s, Z, SCALE, a_, beta, max_iter, in_mode=L.VIT_IN_QPSK, skip=c["Lp"], x=sym.reshape(c["n_bursts"], -1))
        if dec[1][1, 0] >= 1 and dec[1][1, 2] >= 2 and not dec[2].any() and np.array_equal(dec[0], payload_bits_only(LINK_KEY, pay)):
            return (a, b), code, dec
    raise AssertionError("no stretch gives the decoder wrong decisions that it repairs")
