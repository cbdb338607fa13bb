"""What tests/test_fsk_host.py and tests/test_gpu_fsk.py share: the probe configurations and the GPU shapes of the 2-(G)FSK
modem (sfe_dsp_fsk_*), the channel of the round trips, and the law of include/sfe_dsp.h restated in numpy -- uint32 phases and
float32 operations one at a time, every fused operation through synth.fma32 -- for both directions."""
import numpy as np

from simplefe_amd import synth

F32 = np.float32
U32 = np.uint32
PRE24 = [0, 1] * 8 + [0, 0, 1, 1, 0, 1, 0, 0]          # 0101... (16 bits) + 00110100
PRE16 = [0, 1] * 4 + [0, 0, 1, 1, 0, 1, 0, 0]
PRE8 = [0, 1, 0, 1, 0, 0, 1, 1]


def pulse_of(sps, bt=None, span=None, n_rect=None):
    """A Gaussian pulse (bt, span) or a rectangular one of n_rect taps, sum 1."""
    if bt is None:
        n = sps if n_rect is None else n_rect
        return np.full(n, 1.0 / n, F32)
    return synth.gfsk_pulse(bt, sps, span)


def shape(sps, bt=None, span=None, pre=PRE24, n_bits=64, rng=None, h=0.5, amp=1.0, scale=1.0, min_gate=0.0, n_rect=None, out_fmt=0):
    """The keyword arguments of api.fsk_plan / api.Fsk: a boxcar of one symbol as the matched filter (sum 1), delay =
    fsk_delay, R = sps / 2 unless given."""
    g = pulse_of(sps, bt, span, n_rect)
    mf = np.full(sps, 1.0 / sps, F32)
    return dict(sps=sps, pulse=g, h=h, pre=list(pre), n_bits=n_bits, mf=mf, delay=synth.fsk_delay(g.size, mf.size),
                rng=sps // 2 if rng is None else rng, amp=amp, scale=scale, min_gate=min_gate, out_fmt=out_fmt)


# the probe configurations of the issue: (sps, BT, span); BT None: a rectangular pulse of 4 taps
PROBES = [(4, 0.5, 3), (8, 0.5, 3), (10, 0.3, 4), (4, None, None)]
PROBE_IDS = ["sps4-bt0.5", "sps8-bt0.5", "sps10-bt0.3", "sps4-rect"]


def probe(p, **kw):
    sps, bt, span = p
    return shape(sps, bt, span, **kw)


# the GPU shapes: (sps, BT, span, preamble, n_bits, n_bursts)
GPU_SHAPES = [(4, None, None, PRE8, 8, 1), (4, 0.5, 3, PRE24, 64, 5), (8, 0.5, 3, PRE24, 100, 3), (10, 0.3, 4, PRE24, 257, 2),
              (64, 0.5, 2, PRE16, 33, 2), (4, 0.5, 3, PRE24, 2000, 2)]
GPU_IDS = ["sps4-rect-8", "sps4-64x5", "sps8-100x3", "sps10-257x2", "sps64-33x2", "sps4-2000x2"]


def gpu_shape(s, **kw):
    sps, bt, span, pre, n_bits, _ = s
    return shape(sps, bt, span, pre=pre, n_bits=n_bits, **kw)


def payload(n_bits, n_bursts, seed):
    """(n_bursts, ceil(n_bits / 8)) random bytes, pad bits random too (the law ignores them)."""
    return np.random.default_rng(seed).integers(0, 256, size=(int(n_bursts), (int(n_bits) + 7) // 8), dtype=np.uint8)


def payload_clean(n_bits, n_bursts, seed):
    """payload with the pad bits of the last byte 0: what the demodulator's packed bits can return."""
    d = payload(n_bits, n_bursts, seed)
    if n_bits % 8:
        d[:, -1] &= (0xFF << (8 - n_bits % 8)) & 0xFF
    return d


def channel(y, n, at, f=0.01, phase=1.0, snr_db=20.0, seed=0, amp=1.0):
    """The frame y at offset `at` in a zero stream of n samples, a carrier offset of f turns per sample, a phase, complex white
    noise snr_db below amp^2: complex128."""
    rng = np.random.default_rng(seed)
    x = np.zeros(n, np.complex128)
    x[at:at + y.size] = y
    x *= np.exp(2j * np.pi * f * np.arange(n) + 1j * phase)
    if snr_db is not None:
        x += (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5) * amp * 10.0 ** (-snr_db / 20.0)
    return x


# ------------------------------------------------------------------------------------------------ the law in numpy
S = [F32(float.fromhex(v)) for v in ("0x1.921fb6p-1", "-0x1.4abbbap-4", "0x1.465ec4p-9", "-0x1.2d9b7cp-15")]
CC = [F32(float.fromhex(v)) for v in ("-0x1.3bd3ccp-2", "0x1.03c1eap-6", "-0x1.55cb98p-12", "0x1.db64d2p-19")]
AT = [F32(float.fromhex(v)) for v in ("0x1.fffffcp-1", "-0x1.555390p-2", "0x1.995304p-3", "-0x1.2215e6p-3", "0x1.ae613cp-4", "-0x1.28e046p-4",
                                      "0x1.46db72p-5", "-0x1.d9c858p-7", "0x1.43849ep-9")]
PI_2, PI = F32(float.fromhex("0x1.921fb6p+0")), F32(float.fromhex("0x1.921fb6p+1"))


def cis_numpy(p):
    """fsk_cis on an array of uint32 phases: (c, s) float32."""
    p = np.asarray(p, np.uint64) & 0xFFFFFFFF
    q = ((p + (1 << 29)) >> 30) & 3
    r = ((p - (q << 30)) & 0xFFFFFFFF).astype(U32).view(np.int32)
    t = r.astype(F32) * F32(2.0 ** -29)
    z = t * t
    sp = np.full(z.shape, S[3], F32)
    for c in (S[2], S[1], S[0]):
        sp = synth.fma32(sp, z, np.full(z.shape, c, F32))
    s = t * sp
    c = np.full(z.shape, CC[3], F32)
    for k in (CC[2], CC[1], CC[0], F32(1.0)):
        c = synth.fma32(c, z, np.full(z.shape, k, F32))
    co = np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))
    si = np.where(q == 0, s, np.where(q == 1, c, np.where(q == 2, -s, -c)))
    return co.astype(F32), si.astype(F32)


def int_pulse(pulse, h):
    """G (int64) and C (uint32 as uint64 mod 2^32) of a pulse."""
    G = np.rint(np.float64(F32(h)) * np.asarray(pulse, F32).astype(np.float64) * 2.0 ** 31).astype(np.int64)
    C = np.concatenate([[0], np.cumsum(G)]) & 0xFFFFFFFF
    return G, C.astype(np.uint64)


def phases_numpy(kw, bits_row):
    """P[i] of one frame by the defining sum over all k, uint32 arithmetic: (F,) uint64 below 2^32."""
    sps, g = kw["sps"], np.asarray(kw["pulse"], F32)
    _, C = int_pulse(g, kw["h"])
    c = np.concatenate([np.asarray(kw["pre"], np.int64), np.unpackbits(np.asarray(bits_row, np.uint8))[:kw["n_bits"]].astype(np.int64)])
    N, Q = c.size, -(-g.size // sps)
    F = (N + Q - 1) * sps + 1
    i = np.arange(F)[:, None] - np.arange(N)[None, :] * sps
    t = C[np.clip(i, 0, g.size)]
    t = np.where(c[None, :] == 1, (0 - t.astype(np.int64)) & 0xFFFFFFFF, t.astype(np.int64))
    return (t.sum(axis=1) & 0xFFFFFFFF).astype(np.uint64)


def mod_numpy(kw, bits_row):
    """One frame by the law: complex64 (F,)."""
    c, s = cis_numpy(phases_numpy(kw, bits_row))
    amp = F32(kw["amp"])
    y = np.empty(c.size, np.complex64)
    y.real, y.imag = amp * c, amp * s                           # (a sum with 1j would lose the sign of a zero)
    return y


def at2_numpy(y, x):
    """polar_law.h's polar_at2 on float32 arrays."""
    ax, ay = np.abs(x), np.abs(y)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(mx == 0, F32(0), mn / np.where(mx == 0, F32(1), mx)).astype(F32)
    s = z * z
    q = np.full(z.shape, AT[8], F32)
    for c in AT[7::-1]:
        q = synth.fma32(q, s, np.full(z.shape, c, F32))
    r = q * z
    r = np.where(ay > ax, PI_2 - r, r).astype(F32)
    r = np.where(x < 0, PI - r, r).astype(F32)
    return np.where(y < 0, -r, r).astype(F32)


def fm_numpy(x):
    """v[n] for n >= 1 of a complex64 array: polar_sample<POLAR_FM>(x[n], x[n-1], 1)."""
    x = np.asarray(x, np.complex64)
    xr, xi, pr, pi = x.real[1:].astype(F32), x.imag[1:].astype(F32), x.real[:-1].astype(F32), x.imag[:-1].astype(F32)
    re = synth.fma32(xr, pr, xi * pi)
    im = synth.fma32(xi, pr, -(xr * pi))
    return (F32(1.0) * at2_numpy(im, re)).astype(F32)


def tree_numpy(v):
    """The pairwise tree over the last axis: padded with +0 to a power of two, s[k] = s[2k] + s[2k+1] level by level."""
    v = np.asarray(v, F32)
    n2 = 1
    while n2 < v.shape[-1]:
        n2 *= 2
    s = np.zeros(v.shape[:-1] + (n2,), F32)
    s[..., :v.shape[-1]] = v
    while s.shape[-1] > 1:
        s = (s[..., 0::2] + s[..., 1::2]).astype(F32)
    return s[..., 0]


def expected_numpy(kw):
    """(e float32 (Lp,), se, see, den float32) from the integer pulse in float64."""
    sps, m, delay = kw["sps"], np.asarray(kw["mf"], F32).astype(np.float64), kw["delay"]
    G, _ = int_pulse(kw["pulse"], kw["h"])
    a = 1 - 2 * np.asarray(kw["pre"], np.int64)
    Lp = a.size
    D = np.zeros((Lp - 1) * sps + G.size + delay + Lp * sps + m.size, np.float64)
    for k in range(Lp):
        D[k * sps:k * sps + G.size] += a[k] * G
    U = float(G.sum()) / sps * m.sum()
    e = np.array([sum(m[j] * D[delay + k * sps + j - 1] for j in range(m.size)) / U for k in range(Lp)]).astype(F32)
    e64 = e.astype(np.float64)
    se, see = e64.sum(), (e64 * e64).sum()
    return e, F32(se), F32(see), F32(Lp * see - se * se)


def demod_numpy(kw, x, o):
    """One burst whose reach is inside x (complex64) by steps 2-6 of the law in float32: (soft, bytes, record, status)."""
    sps, m, delay, R, n_bits = kw["sps"], np.asarray(kw["mf"], F32), kw["delay"], kw["rng"], kw["n_bits"]
    e, se, see, den = expected_numpy(kw)
    Lp, N = e.size, e.size + n_bits
    lo, hi = o + delay - R - 1, o + delay + R + (N - 1) * sps + m.size
    fail = (np.zeros(n_bits, F32), np.zeros((n_bits + 7) // 8, np.uint8), np.array([np.nan] * 4 + [0.0] * 4, F32), 1)
    seg = np.asarray(x, np.complex64)[lo:hi]
    if not (np.isfinite(seg.real).all() and np.isfinite(seg.imag).all()):
        return fail
    v = fm_numpy(seg)                                           # v[i] is the law's v[delay - R + i]

    def u(idx):                                                 # idx: the law's i - (delay - R), any shape
        acc = np.zeros(np.shape(idx), F32)
        for j in range(m.size):
            acc = synth.fma32(np.full(acc.shape, m[j], F32), v[np.asarray(idx) + j], acc)
        return acc

    taus = np.arange(-R, R + 1)
    uk = u(R + taus[:, None] + np.arange(Lp)[None, :] * sps)    # (2R + 1, Lp)
    S1, Se = tree_numpy(uk), tree_numpy((e[None, :] * uk).astype(F32))
    num = synth.fma32(np.full(S1.shape, F32(Lp), F32), Se, -(se * S1).astype(F32))
    ok = ~np.isnan(num)
    if not ok.any():
        return fail
    best = int(np.flatnonzero(ok & (num == num[ok].max()))[0])
    tau = int(taus[best])
    dev = F32(num[best] / den)
    if not (dev > 0 and np.isfinite(dev)):
        return fail
    dc = F32(F32(S1[best] - F32(dev * se)) / F32(Lp))
    f = F32(dc * F32(float.fromhex("0x1.45f306p-3")))
    d = (uk[best] - synth.fma32(np.full(Lp, dev, F32), e, np.full(Lp, dc, F32))).astype(F32)
    q = F32(tree_numpy((d * d).astype(F32)) / F32(F32(dev * dev) * see))
    ud = u(R + tau + (Lp + np.arange(n_bits)) * sps)
    soft = (F32(kw["scale"]) * ((ud - dc).astype(F32) / dev).astype(F32)).astype(F32)
    by = np.packbits((soft < 0).astype(np.uint8))
    return soft, by, np.array([tau, f, dev, q, 0, 0, 0, 0], F32), 0


def f32_as_u8_samples(x):
    """A cf32 stream as the receive wire format's (I,Q) bytes, and those bytes converted back as the device converts them."""
    b = synth.f32_to_u8(np.asarray(x, np.complex64))
    return b, synth.u8_to_cf32(b)
