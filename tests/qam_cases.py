"""What tests/test_qam_host.py and tests/test_gpu_qam.py share: shapes and inputs of the QAM mapper and soft demapper
(sfe_dsp_qam_*), a restatement of its law in numpy float32, one operation at a time, and the chain
payload -> ldpc (encode) -> qam (map) -> ofdmmod (SYMBOLS) -> a two-tap channel and noise -> ofdm (ZF, chan) -> qam (demap,
CSI) -> ldpc (decode) through the host plans.  Host only: numpy, simplefe_amd.synth and the plans; nothing here touches a
GPU."""
import functools

import numpy as np

import ldpc_cases as lc
import ofdm_cases as oc
import ofdmmod_cases as mc
from simplefe_amd import synth

F32 = np.float32
ORDERS = (2, 4, 16, 64, 256)
BPS = {2: 1, 4: 2, 16: 4, 64: 6, 256: 8}


def axis_bits(order):
    return 1 if order == 2 else BPS[order] // 2


def perm_of(kind, B, seed=0):
    """None, the reversal, or a seeded random permutation of [0, B)."""
    if kind is None or kind == "none":
        return None
    if kind == "reversal":
        return np.arange(B - 1, -1, -1, dtype=np.uint32)
    return np.random.default_rng(synth.SEED + 7000 + seed).permutation(B).astype(np.uint32)


def csi_of(period, n_rows, seed=0):
    """(csi_index uint32 [period] or None, csi_len, csi (n_rows, csi_len) complex64 or None): period 52 reads 64 bins the way
    an OFDM shape does (increasing, with gaps), the others read a table of their own length in a seeded order."""
    if not period:
        return None, 0, None
    rng = np.random.default_rng(synth.SEED + 8000 + seed + period)
    if period == 52:
        clen = 64
        idx = np.sort(rng.choice(clen, size=period, replace=False)).astype(np.uint32)
    else:
        clen = period
        idx = rng.permutation(period).astype(np.uint32)
    h = (0.2 + rng.random((n_rows, clen))) * np.exp(2j * np.pi * rng.random((n_rows, clen)))
    return idx, clen, h.astype(np.complex64)


def coded_bytes(n_rows, n_bytes, seed=0, pad=0):
    return np.random.default_rng(synth.SEED + 9000 + seed).integers(0, 256, size=(n_rows, n_bytes + pad), dtype=np.uint8)


def noisy_symbols(order, n_rows, n_sym, amp=1.0, noise=0.3, seed=0):
    """Points of the constellation drawn at random plus Gaussian noise of `noise` level spacings, complex64 (n_rows, n_sym)."""
    rng = np.random.default_rng(synth.SEED + 9500 + seed + order)
    pts, _ = synth.qam_points(order, amp)
    lev = synth.qam_levels(order, amp).astype(np.float64)
    step = 2.0 * float(np.abs(lev).min())
    z = pts[rng.integers(0, pts.size, size=(n_rows, n_sym))]
    return (z + noise * step * (rng.standard_normal(z.shape) + 1j * rng.standard_normal(z.shape))).astype(np.complex64)


def law_numpy(sym, order, amp=1.0, scale=1.0, perm=None, csi=None, csi_index=None):
    """The law of include/sfe_dsp.h in np.float32, one operation at a time: (n_rows, n_sym bps) float32."""
    z = np.atleast_2d(np.asarray(sym, np.complex64))
    nr, ns = z.shape
    bps, m = BPS[order], axis_bits(order)
    K = 1 if order == 2 else 2 * (order - 1) // 3
    u, wbits = synth.qam_axis_words(m)
    lev = (np.float64(F32(amp)) * u.astype(np.float64) / np.sqrt(np.float64(K))).astype(F32)
    w = np.full((nr, ns), F32(scale), F32)
    if csi_index is not None:
        idx = np.asarray(csi_index, np.int64)
        h = np.atleast_2d(np.asarray(csi, np.complex64))[:, idx[np.arange(ns) % idx.size]]
        hr, hi = h.real.astype(F32), h.imag.astype(F32)
        p = (hr * hr).astype(F32)
        g = (hi.astype(np.longdouble) * hi.astype(np.longdouble) + p.astype(np.longdouble)).astype(F32)      # fmaf: the exact sum (see below), rounded once
        w = (F32(scale) * g).astype(F32)
    out = np.empty((nr, ns, bps), F32)
    for ax, y in enumerate((z.real.astype(F32), z.imag.astype(F32))[:1 if bps == 1 else 2]):
        t = (y[..., None] - lev[None, None, :]).astype(F32)
        e = (t * t).astype(F32)
        for c in range(m):
            one = wbits[:, c] == 1
            d0, d1 = e[..., ~one].min(axis=-1), e[..., one].min(axis=-1)
            d = (d1 - d0).astype(F32)
            out[..., ax * m + c] = (w * d).astype(F32)
    out = out.reshape(nr, ns * bps)
    if perm is not None:
        sc = np.empty_like(out)
        sc[:, np.asarray(perm, np.int64)] = out
        out = sc
    return out


# hi * hi + p is exact in the 64-bit significand of x86's long double while the two terms lie within 2^16 of each other (a
# 48-bit product beside a 24-bit one): everywhere in these tests |h|'s components are far inside that.
assert np.finfo(np.longdouble).nmant >= 63


# ---- the chain on the n64 OFDM shape with three data symbols: code B of tests/ldpc_cases.py, n = 648 = 162 symbols of
# 16-QAM = 3 x 54 data bins.  A fixed two-tap channel whose second tap is nearly as strong as the first, so that some data bins
# lie in a null; fixed-seed noise.  CHAIN_NOISE was chosen on the CPU through the host plans (chain_on_the_cpu asserts what it
# was chosen for): with the |H|^2 weighting every codeword converges to its payload, without it at least one does not.
CHAIN = dict(order=16, n_words=4, n_data=3, taps={0: 1.0, 2: 0.9 * np.exp(0.4j)}, gap=23, qam_scale=16.0, seed=11)
CHAIN_NOISE = 0.016


def chain_shapes():
    """(ofdmmod keyword arguments, ofdm keyword arguments, csi_index, perm) of the chain."""
    c = CHAIN
    tx = mc.shape_args("n64", amp=1.0, in_mode=mc.SYMBOLS, n_data=c["n_data"])
    rx = oc.shape_args("n64", 0, 0.0)
    rx["n_data"] = c["n_data"]
    rx["pilot_sign"] = tx["pilot_sign"]
    csi_index = np.flatnonzero(np.asarray(tx["kind"]) == 1).astype(np.uint32)
    return tx, rx, csi_index, perm_of("random", 648, 5)


def chain_channel(wave, noise):
    """The waveform through the two taps, plus complex Gaussian noise of standard deviation `noise` per component."""
    c = CHAIN
    h = np.zeros(max(c["taps"]) + 1, np.complex128)
    for d, v in c["taps"].items():
        h[d] = v
    y = np.convolve(wave.astype(np.complex128), h)[:wave.size]
    rng = np.random.default_rng(synth.SEED + 4300 + c["seed"])
    return (y + noise * (rng.standard_normal(y.size) + 1j * rng.standard_normal(y.size))).astype(np.complex64)


def chain_decode(api, L, llr):
    s, Z = lc.CASES["B"]
    a_, beta, max_iter = lc.PARAMS["a12"]
    return api.ldpc_plan(s, Z, lc.SCALE, a_, beta, max_iter, in_mode=L.VIT_IN_SOFT, x=llr)


def chain_on_the_cpu(api, L, noise=None, check=True):
    """The chain through the host plans.  Returns a dict: pay, code, sym (the mapper's rows), wave (the modulator's stream),
    x (what the receiver reads), starts (base, step), z and chan (the receiver's rows), llr, llr_flat (demapped without CSI),
    dec and dec_flat (ldpc_plan's answers to the two)."""
    c = CHAIN
    noise = CHAIN_NOISE if noise is None else noise
    tx, rx, csi_index, perm = chain_shapes()
    s, Z = lc.CASES["B"]
    nw = c["n_words"]
    pay = lc.payloads("B", nw, 91)
    code = api.ldpc_plan(s, Z, data=pay)
    sym = api.qam_plan(c["order"], 162, perm=perm, data=code)
    F = mc.sizes(tx)[3]
    base, step = 5, F + c["gap"]
    n_out = base + nw * step
    wave = api.ofdmmod_plan(**tx, data=sym, n_out=n_out, start_base=base, start_step=step)
    x = chain_channel(wave, noise)
    z, chan, rec, st = api.ofdm_plan(x=x, n_bursts=nw, start_base=base, start_step=step, **rx)
    z = z.reshape(nw, -1)
    kw = dict(scale=c["qam_scale"], perm=perm)
    llr = api.qam_plan(c["order"], 162, csi_index=csi_index, csi_len=64, sym=z, csi=chan, **kw)
    llr_flat = api.qam_plan(c["order"], 162, sym=z, **kw)
    dec, dec_flat = chain_decode(api, L, llr), chain_decode(api, L, llr_flat)
    out = dict(pay=pay, code=code, sym=sym, wave=wave, x=x, starts=(base, step), n_out=n_out, z=z, chan=chan, st=st, llr=llr, llr_flat=llr_flat,
               dec=dec, dec_flat=dec_flat, min_h2=float((np.abs(chan[:, csi_index]) ** 2).min() / (np.abs(chan[:, csi_index]) ** 2).mean()))
    if check:
        want = lc.payload_bits_only("B", pay)
        assert not st.any()
        assert not dec[2].any() and np.array_equal(dec[0], want), (dec[2], dec[1])
        bad = [i for i in range(nw) if dec_flat[2][i] != 0 or not np.array_equal(dec_flat[0][i], want[i])]
        assert bad, "the unweighted demapper decodes every word too: the weighting is not seen to matter"
        out["bad_flat"] = bad
    return out


@functools.lru_cache(maxsize=None)
def _chain_cached(noise):
    from simplefe_amd import api, lib
    return chain_on_the_cpu(api, lib, noise)


def chain(noise=None):
    """chain_on_the_cpu's answer, computed once."""
    return _chain_cached(CHAIN_NOISE if noise is None else noise)
