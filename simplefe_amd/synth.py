"""Deterministic synthetic I/Q streams and filter prototypes.

The sample generator is a counter-based 32-bit hash, defined once here and implemented
identically on the device (csrc/synth.hip: sfe_dsp_synth_fill), so a 2^30-sample stream
can be generated in HBM and any window of it reproduced on the host for checking.
Values are (int32(hash) >> 8) * 2^-23: exactly representable float32 in [-1, 1).
"""
import os

import numpy as np

SEED = 20240601

_M32 = np.uint64(0xFFFFFFFF)


def hash32(seed, ch, idx):
    """lowbias32-style finaliser over (seed, channel, 64-bit float index)."""
    idx = np.asarray(idx, dtype=np.uint64)
    lo = idx & _M32
    hi = idx >> np.uint64(32)
    x = (lo * np.uint64(0x9E3779B9) + hi * np.uint64(0x7F4A7C15)
         + np.uint64(int(seed) & 0xFFFFFFFF) * np.uint64(0x85EBCA6B)
         + np.uint64(int(ch) & 0xFFFFFFFF) * np.uint64(0xC2B2AE35)
         + np.uint64(0x165667B1)) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def synth_f32(n_floats, seed=SEED, ch=0, first=0):
    """n_floats float32 values; float index i of channel ch is hash32(seed, ch, first+i)."""
    idx = np.arange(first, first + n_floats, dtype=np.uint64)
    u = hash32(seed, ch, idx)
    return (u.view(np.int32) >> 8).astype(np.float32) * np.float32(2.0 ** -23)


def synth_cf32(n_samples, seed=SEED, ch=0, first_sample=0):
    """Interleaved (re, im) float32 array of 2*n_samples floats (gr_complex layout,
    gr-simplefe/lib/source_c_impl.cc:46)."""
    return synth_f32(2 * n_samples, seed, ch, 2 * first_sample)


def lowpass_taps(n_taps, cutoff, gain=1.0):
    """Hamming-windowed sinc, computed in float64 and rounded to float32.
    cutoff is a fraction of Nyquist; DC gain is `gain`."""
    k = np.arange(n_taps, dtype=np.float64) - (n_taps - 1) / 2.0
    h = np.sinc(cutoff * k) * (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(n_taps) / max(n_taps - 1, 1)))
    h *= gain / h.sum()
    return h.astype(np.float32)


def complex_taps(n_taps, cutoff, shift=0.1):
    """The same prototype shifted by e^{j*shift*pi*k}: returns (re, im) float32 arrays."""
    h = lowpass_taps(n_taps, cutoff).astype(np.float64)
    k = np.arange(n_taps)
    w = np.exp(1j * shift * np.pi * k)
    return (h * w.real).astype(np.float32), (h * w.imag).astype(np.float32)


# BASELINE.json configs
def taps_cfg1():
    return lowpass_taps(63, 0.25)


def taps_cfg2():
    return lowpass_taps(256, 0.2)


def taps_per_channel(n_channels, n_taps=256):
    """cfg5's "per-channel-distinct taps" variant: channel c's 256-tap Hamming
    windowed-sinc low-pass at cut-off 0.10 + 0.30 c / n_channels (float64 formula, rounded to float32)."""
    k = np.arange(n_taps, dtype=np.float64) - (n_taps - 1) / 2.0
    w = 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(n_taps) / (n_taps - 1))
    out = np.empty((n_channels, n_taps), dtype=np.float32)
    for c in range(n_channels):
        fc = 0.10 + 0.30 * c / n_channels
        h = fc * np.sinc(fc * k) * w
        out[c] = (h / h.sum()).astype(np.float32)
    return out


def taps_cfg3():
    """381-tap prototype for U=3 (127 taps per polyphase arm), rate 5/3, DC gain U."""
    return lowpass_taps(381, 0.18, gain=3.0)


def taps_cfg3_short():
    """The other reading of configs[2]: a 127-tap PROTOTYPE for U=3 (43 taps per
    polyphase arm), same cutoff and gain."""
    return lowpass_taps(127, 0.18, gain=3.0)


def taps_cfg4():
    return lowpass_taps(64, 0.9 / 8.0)


def rel_rms(y, ref):
    y = np.asarray(y, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    den = np.sqrt(np.sum(ref * ref))
    return float(np.sqrt(np.sum((y - ref) ** 2)) / den) if den > 0 else float(np.sqrt(np.sum(y * y)))


def chan_reference(x, h, n_chans, decim, first=0):
    """The channelizer's contract (sfe_dsp_chan_*) computed literally in float64, channel by channel: mix x down by
    exp(-j 2 pi k i / M) (i the absolute sample index, x[0] being sample `first`), convolve with h (FFT convolution;
    samples before x[0] are zero), keep the samples at i = m * decim.  Returns (M, n_out) complex128 for the instants
    m * decim in [first, first + len(x))."""
    x = np.asarray(x).astype(np.complex128).ravel()
    h = np.asarray(h, dtype=np.float64).ravel()
    M, D, n = int(n_chans), int(decim), x.size
    i = first + np.arange(n)
    keep = np.nonzero(i % D == 0)[0]
    try:                                    # batched transforms on several cores where scipy is installed
        from scipy import fft as F
        kw = {"workers": min(16, os.cpu_count() or 1)}
    except ImportError:
        F, kw = np.fft, {}
    nfft = 1 << int(np.ceil(np.log2(n + h.size)))
    H = F.fft(h, nfft)
    mix = np.exp(-2j * np.pi * np.arange(M) / M)          # exp(-j 2 pi q / M), indexed by (k i) mod M
    out = np.empty((M, keep.size), dtype=np.complex128)
    for k0 in range(0, M, 16):
        k = np.arange(k0, min(M, k0 + 16))[:, None]
        z = x[None, :] * mix[(k * (i % M)[None, :]) % M]
        out[k0:k0 + k.shape[0]] = F.ifft(F.fft(z, nfft, axis=1, **kw) * H[None, :], axis=1, **kw)[:, keep]
    return out


def chan_reference_direct(x, h, n_chans, decim, first, m0, n_out):
    """The same contract evaluated straight from its formula, for windows of long streams: outputs m0 .. m0+n_out-1,
    y_k[m] = sum_n h[n] x[mD - n] exp(-j 2 pi k (mD - n) / M), with x[0] being sample `first` (which must be
    <= m0 D - (len(h) - 1), or 0).  One matrix product per window: rows are instants, columns taps."""
    x = np.asarray(x).astype(np.complex128).ravel()
    h = np.asarray(h, dtype=np.float64).ravel()
    M, D, L = int(n_chans), int(decim), h.size
    m = m0 + np.arange(n_out)
    idx = (m * D)[:, None] - np.arange(L)[None, :] - first         # [n_out, L] positions in x
    X = np.where(idx >= 0, x[np.clip(idx, 0, None)], 0)
    if first > 0:
        assert idx.min() >= 0, "the window must hold the L-1 samples before its first output"
    n = np.arange(L)
    k = np.arange(M)
    G = h[:, None] * np.exp(2j * np.pi * ((n[:, None] * k[None, :]) % M) / M)             # [L, M]
    lead = np.exp(-2j * np.pi * (((m * D)[:, None] % M) * k[None, :] % M) / M)          # [n_out, M]
    return ((X @ G) * lead).T


def ddc_incs(freqs):
    """The down-converter's quantised NCO increments: llround(f 2^32) mod 2^32 (sfe_dsp_ddc_plan)."""
    v = np.atleast_1d(np.asarray(freqs, dtype=np.float64)) * 2.0 ** 32
    return [int(np.sign(a) * np.floor(abs(a) + 0.5)) % (1 << 32) for a in v]          # llround: halves away from zero


def _ddc_phase(i, inc):
    """exp(-j 2 pi ((i inc) mod 2^32) / 2^32) for integer sample indices i (numpy int64), exactly in the integer phase."""
    ph = (np.asarray(i, dtype=np.int64) % (1 << 32)).astype(np.uint64) * np.uint64(inc) % np.uint64(1 << 32)
    return np.exp(-2j * np.pi * ph.astype(np.float64) / 2.0 ** 32)


def ddc_reference(x, h, decim, incs, first=0):
    """The down-converter bank's contract (sfe_dsp_ddc_*) in float64, tuning by tuning: mix x down by exp(-j 2 pi
    phi_k(i) / 2^32) with the exact integer phase (i the absolute sample index, x[0] being sample `first`), convolve with h
    (FFT convolution; samples before x[0] are zero), keep i = m * decim.  Returns (K, n_out) complex128 for the instants
    m * decim in [first, first + len(x))."""
    x = np.asarray(x).astype(np.complex128).ravel()
    h = np.asarray(h, dtype=np.float64).ravel()
    D, n = int(decim), x.size
    i = first + np.arange(n)
    keep = np.nonzero(i % D == 0)[0]
    nfft = 1 << int(np.ceil(np.log2(n + h.size)))
    H = np.fft.fft(h, nfft)
    out = np.empty((len(incs), keep.size), dtype=np.complex128)
    for k, inc in enumerate(incs):
        out[k] = np.fft.ifft(np.fft.fft(x * _ddc_phase(i, inc), nfft) * H)[keep]
    return out


def ddc_reference_direct(x, h, decim, incs, first, m0, n_out):
    """The same contract evaluated straight from its formula, for windows of long streams: outputs m0 .. m0+n_out-1,
    y_k[m] = sum_n h[n] x[mD - n] exp(-j 2 pi phi_k(mD - n) / 2^32), with x[0] being sample `first` (which must be
    <= m0 D - (len(h) - 1), or 0).  One matrix product per tuning: rows are instants, columns taps."""
    x = np.asarray(x).astype(np.complex128).ravel()
    h = np.asarray(h, dtype=np.float64).ravel()
    D, L = int(decim), h.size
    m = m0 + np.arange(n_out, dtype=np.int64)
    idx = (m * D)[:, None] - np.arange(L)[None, :] - first            # [n_out, L] positions in x
    X = np.where(idx >= 0, x[np.clip(idx, 0, None)], 0)
    if first > 0:
        assert idx.min() >= 0, "the window must hold the L-1 samples before its first output"
    out = np.empty((len(incs), n_out), dtype=np.complex128)
    for k, inc in enumerate(incs):
        out[k] = (X * _ddc_phase(idx + first, inc)) @ h
    return out


def combine_reference(X, g, n_chans, interp, first=0):
    """The combiner's contract (sfe_dsp_combine_*) in float64: X is (M, n) complex, the channel inputs of instants
    first .. first+n-1 (earlier instants are zero).  v = M * ifft(X) over the channels gives v_q[m] =
    sum_k X_k[m] exp(+j 2 pi k q / M); each instant m then adds g[t] * v_{(mD + t) mod M}[m] to output sample mD + t
    (overlap-add, t < L).  Returns the n*D complex128 samples [first*D, (first+n)*D)."""
    X = np.asarray(X).astype(np.complex128)
    g = np.asarray(g, dtype=np.float64).ravel()
    M, D, L = int(n_chans), int(interp), g.size
    n = X.shape[1]
    v = np.fft.ifft(X, axis=0) * M                                   # [M, n]
    z = np.zeros(n * D + L, dtype=np.complex128)
    t = np.arange(L)
    for m in range(n):
        z[m * D:m * D + L] += g * v[((first + m) * D + t) % M, m]
    return z[:n * D]


def combine_reference_direct(X, g, n_chans, interp, first, i0, n_out):
    """The same contract evaluated from its formula for a window of a long stream: outputs i0 .. i0+n_out-1 (absolute),
    z[i] = sum_m g[i - mD] sum_k X_k[m] exp(+j 2 pi k i / M), with X (M, n) holding instants first .. first+n-1 (which
    must include every instant the window reaches, or start at 0).  The channel sums are an explicit DFT matrix
    product, the taps a gather per output phase: no FFT."""
    X = np.asarray(X).astype(np.complex128)
    g = np.asarray(g, dtype=np.float64).ravel()
    M, D, L = int(n_chans), int(interp), g.size
    i = i0 + np.arange(n_out)
    m_lo = -(-(i0 - L + 1) // D)                                     # ceil: the earliest instant the window reaches
    if first > 0:
        assert first <= max(m_lo, 0), "the window must hold every instant its outputs reach"
    m_hi = (i0 + n_out - 1) // D
    ms = np.arange(max(m_lo, first), m_hi + 1)
    k = np.arange(M)
    E = np.exp(2j * np.pi * ((k[:, None] * k[None, :]) % M) / M)    # [k, q]
    V = E.T @ X[:, ms - first]                                       # [q, m]: v_q[m]
    z = np.zeros(n_out, dtype=np.complex128)
    for j in range(-(-L // D)):
        m = i // D - j
        tap = i - m * D
        ok = (tap < L) & (m >= ms[0]) & (m <= ms[-1])
        z[ok] += g[tap[ok]] * V[i[ok] % M, m[ok] - ms[0]]
    return z


def psd_rows(n, n_fft, hop, n_avg, first=0):
    """The rows of the spectrum estimator (sfe_dsp_psd_*) that samples [first, first + n) hold whole: (r_lo, r_hi),
    rows r_lo <= r < r_hi.  Segment m reads samples [(m + 1) H - N, (m + 1) H); a stream that starts at sample 0 has zeros
    before it, one that starts later must hold every sample of a row's first segment."""
    N, H, A = int(n_fft), int(hop), int(n_avg)
    m_lo = 0 if first == 0 else max(0, -(-(first + N) // H) - 1)      # the first m with (m + 1) H - N >= first
    r_lo = -(-m_lo // A)
    return r_lo, max(r_lo, ((first + n) // H) // A)


def psd_reference(x, w, hop, n_avg, scale, first=0):
    """The spectrum estimator's contract (sfe_dsp_psd_*) in float64 through np.fft.fft: x[0] is absolute sample `first`
    (zeros before it when first = 0); segment m is the N samples that end at (m + 1) hop, times the window w; row r is
    scale times the sum of |fft|^2 over segments [r n_avg, (r + 1) n_avg).  Returns (rows, N) float64 for the rows
    psd_rows(len(x), N, hop, n_avg, first) names."""
    x = np.asarray(x).astype(np.complex128).ravel()
    w = np.asarray(w, dtype=np.float64).ravel()
    N, H, A = w.size, int(hop), int(n_avg)
    r_lo, r_hi = psd_rows(x.size, N, H, A, first)
    try:                                    # batched transforms on several cores where scipy is installed
        from scipy import fft as F
        kw = {"workers": min(16, os.cpu_count() or 1)}
    except ImportError:
        F, kw = np.fft, {}
    xp = np.concatenate([np.zeros(N, dtype=np.complex128), x]) if first == 0 else x
    off = N if first == 0 else -first       # position in xp of absolute sample 0
    out = np.empty((r_hi - r_lo, N), dtype=np.float64)
    for r in range(r_lo, r_hi):
        b = (np.arange(r * A, (r + 1) * A) + 1) * H - N + off
        seg = xp[b[:, None] + np.arange(N)[None, :]] * w[None, :]
        X = F.fft(seg, axis=1, **kw)
        out[r - r_lo] = scale * np.sum(X.real ** 2 + X.imag ** 2, axis=0)
    return out


def psd_reference_direct(x, w, hop, n_avg, scale, first, row, bins):
    """The same contract with the DFT sum written out, for chosen bins of one absolute row: out[k] = scale sum_m
    |sum_n w[n] x[(m + 1) hop - N + n] exp(-j 2 pi k n / N)|^2 over the row's segments, x[0] being absolute sample
    `first` (which must be 0 or at most the row's first sample).  One matrix product per row: no FFT, no shared framing
    code with psd_reference."""
    x = np.asarray(x).astype(np.complex128).ravel()
    w = np.asarray(w, dtype=np.float64).ravel()
    N, H, A = w.size, int(hop), int(n_avg)
    k = np.asarray(bins, dtype=np.int64)
    n = np.arange(N)
    E = w[:, None] * np.exp(-2j * np.pi * ((n[:, None] * k[None, :]) % N) / N)          # [N, bins]
    acc = np.zeros(k.size, dtype=np.float64)
    for m in range(row * A, (row + 1) * A):
        idx = (m + 1) * H - N + n - first
        if first > 0:
            assert idx[0] >= 0, "the window must hold the row's first sample"
        seg = np.where(idx >= 0, x[np.clip(idx, 0, None)], 0)
        acc += np.abs(seg @ E) ** 2
    return scale * acc


def _corr_frame(x, templates, first):
    """x and the templates as complex128, with the L - 1 zeros a stream that starts at sample 0 has before it."""
    x = np.asarray(x).astype(np.complex128).ravel()
    t = np.atleast_2d(np.asarray(templates).astype(np.complex128))
    L = t.shape[1]
    if first == 0:
        x = np.concatenate([np.zeros(L - 1, dtype=np.complex128), x])
    return x, t, L


def corr_reference(x, templates, block, min_energy, first=0):
    """The correlator bank's contract (sfe_dsp_corr_*) in float64: the returned values are those of absolute samples
    first, first + 1, ..., `first` a multiple of block.  With first = 0, x[0] is sample 0 and zeros precede it; otherwise
    x starts with the L - 1 samples before `first`, so every returned value has its whole window.  c_k is the
    convolution with conj(s_k) reversed (np.convolve; through float64 transforms for templates longer than 64), the
    window energy e np.convolve of |x|^2 with L ones (a direct sum, no differenced cumsum), m_k = |c_k|^2 / (E_k e)
    where e > min_energy, else 0.  Returns (m (K, n) float64, peak_val (K, n // block), peak_idx (K, n // block) int64:
    the first arg-maximum of each block)."""
    assert first % int(block) == 0
    xp, t, L = _corr_frame(x, templates, first)
    n = xp.size - (L - 1)
    e = np.convolve(xp.real ** 2 + xp.imag ** 2, np.ones(L), mode="valid")
    m = np.zeros((t.shape[0], n), dtype=np.float64)
    ok = e > min_energy
    nfft = 1 << int(np.ceil(np.log2(xp.size + L)))
    X = np.fft.fft(xp, nfft) if L > 64 else None
    for k in range(t.shape[0]):
        h = np.conj(t[k])[::-1]
        c = np.convolve(xp, h, mode="valid") if X is None else np.fft.ifft(X * np.fft.fft(h, nfft))[L - 1:L - 1 + n]
        E = float(np.sum(t[k].real ** 2 + t[k].imag ** 2))
        m[k, ok] = (c.real[ok] ** 2 + c.imag[ok] ** 2) / (E * e[ok])
    nb = n // int(block)
    blocks = m[:, :nb * int(block)].reshape(t.shape[0], nb, int(block))
    return m, blocks.max(axis=2), blocks.argmax(axis=2)


def corr_reference_direct(x, templates, min_energy, first, points):
    """The same contract by the explicit double loop, for chosen (k, i) with i absolute: no convolution, no shared
    framing code with corr_reference.  x[0] is absolute sample `first`; samples before absolute 0 are zero, and with
    first > 0 every window must lie inside x."""
    x = np.asarray(x).astype(np.complex128).ravel()
    t = np.atleast_2d(np.asarray(templates).astype(np.complex128))
    L = t.shape[1]
    out = []
    for k, i in points:
        c, e, E = 0.0 + 0.0j, 0.0, 0.0
        for n in range(L):
            a = i - (L - 1) + n
            E += abs(t[k, n]) ** 2
            if a < 0:
                continue
            assert a - first >= 0, "the window must lie inside x"
            v = x[a - first]
            c += np.conj(t[k, n]) * v
            e += abs(v) ** 2
        out.append(abs(c) ** 2 / (E * e) if e > min_energy else 0.0)
    return np.array(out)


# ---- the biquad-cascade IIR filter (sfe_dsp_iir_*): designers that return float64 sos rows (b0, b1, b2, a0, a1, a2), the
# float32 coefficients of the law, and the law itself sample by sample
def iir_dc_blocker(r):
    """y[i] = x[i] - x[i-1] + r y[i-1]: a zero at DC, a pole at radius r."""
    return np.array([[1.0, -1.0, 0.0, 1.0, -float(r), 0.0]])


def iir_one_pole(a):
    """y[i] = (1 - a) x[i] + a y[i-1]: unit DC gain."""
    return np.array([[1.0 - float(a), 0.0, 0.0, 1.0, -float(a), 0.0]])


def iir_notch(f0, q):
    """The RBJ cookbook notch at f0 cycles per sample with quality q."""
    w0 = 2.0 * np.pi * float(f0)
    al = np.sin(w0) / (2.0 * float(q))
    return np.array([[1.0, -2.0 * np.cos(w0), 1.0, 1.0 + al, -2.0 * np.cos(w0), 1.0 - al]])


def iir_butter_lowpass(order, fc):
    """Butterworth low-pass of even `order`, -3 dB at fc cycles per sample: order / 2 RBJ low-pass sections with
    Q_k = 1 / (2 sin((2k + 1) pi / (2 order)))."""
    order = int(order)
    if order < 2 or order % 2:
        raise ValueError("iir_butter_lowpass: order must be even and >= 2")
    w0 = 2.0 * np.pi * float(fc)
    c, s = np.cos(w0), np.sin(w0)
    rows = []
    for k in range(order // 2):
        al = s * np.sin((2 * k + 1) * np.pi / (2.0 * order))       # sin(w0) / (2 Q_k)
        rows.append([(1.0 - c) / 2.0, 1.0 - c, (1.0 - c) / 2.0, 1.0 + al, -2.0 * c, 1.0 - al])
    return np.array(rows)


def iir_round(sos):
    """The float32 values the law is stated on: (S, 5) rows (B0, B1, B2, A1, A2) = the sos rows divided by a0 in
    float64, each rounded once."""
    sos = np.atleast_2d(np.asarray(sos, dtype=np.float64))
    return (sos[:, [0, 1, 2, 4, 5]] / sos[:, 3:4]).astype(np.float32)


def iir_reference(x, sos, dtype=np.float64):
    """The law of sfe_dsp_iir_* sample by sample on the rounded coefficients, zero state before x[0].  x is (..., n) real
    or complex (I and Q never mix); the result has x's shape, float64 / complex128.  With dtype=np.float32 every product
    and every sum is rounded to float32, in the order ((B0 v[i] + B1 v[i-1]) + B2 v[i-2]) - A1 y[i-1] - A2 y[i-2]: the
    yardstick of what float32 itself makes of the recursion."""
    x = np.asarray(x)
    cplx = np.iscomplexobj(x)
    v = x.astype(np.complex128).view(np.float64).reshape(x.shape + (2,)) if cplx else x.astype(np.float64)[..., None]
    n = x.shape[-1]
    v = np.moveaxis(v, -2, 0).reshape(n, -1)                # (n, columns): time first
    c32 = iir_round(sos)
    if dtype == np.float64:
        try:                                # the same recursion compiled, where scipy is installed
            from scipy.signal import sosfilt
            c = c32.astype(np.float64)
            rows = np.ascontiguousarray(np.concatenate([c[:, :3], np.ones((c.shape[0], 1)), c[:, 3:]], axis=1))
            y = sosfilt(rows, v, axis=0)
        except ImportError:
            y = _iir_loop(v, c32.astype(np.float64), np.float64)
    else:
        y = _iir_loop(v.astype(np.float32), c32, np.float32).astype(np.float64)
    y = np.moveaxis(y.reshape((n,) + x.shape[:-1] + (2 if cplx else 1,)), 0, -2)
    return np.ascontiguousarray(y).view(np.complex128)[..., 0] if cplx else y[..., 0]


def _iir_loop(v, coef, dt):
    """(n, columns) through the cascade; every operation in dt."""
    n = v.shape[0]
    for b0, b1, b2, a1, a2 in coef.astype(dt):
        w = b0 * v                                          # the feed-forward part has no recursion: whole columns at once
        if b1 != 0:
            w[1:] = w[1:] + b1 * v[:-1]
        if b2 != 0:
            w[2:] = w[2:] + b2 * v[:-2]
        y = np.empty_like(w)
        y1 = y2 = np.zeros(v.shape[1], dt)
        for i in range(n):
            t = w[i] - a1 * y1
            if a2 != 0:
                t = t - a2 * y2
            y[i] = t
            y2, y1 = y1, t
        v = y
    return v


def iir_grid_filters():
    """The filters the IIR tests and scripts/time_iir.py share, by name: S = 1, 1, 1, 1, 2, 8 and 5 sections."""
    return {"dc(0.995)": iir_dc_blocker(0.995), "dc(0.9999)": iir_dc_blocker(0.9999), "notch(0.125,30)": iir_notch(0.125, 30.0),
            "notch(0.125,1000)": iir_notch(0.125, 1000.0), "butter(4,0.025)": iir_butter_lowpass(4, 0.025),
            "butter(16,0.1)": iir_butter_lowpass(16, 0.1),
            "dc(0.999)+butter(8,0.1)": np.vstack([iir_dc_blocker(0.999), iir_butter_lowpass(8, 0.1)])}


# ---- the FM, phase and envelope detector (sfe_dsp_polar_*)
POLAR_FM, POLAR_PM, POLAR_AM = 0, 1, 2


def polar_reference(x, mode, gain=1.0, prev=0.0):
    """The law of sfe_dsp_polar_* in float64 on the samples as given: x is (..., n) complex; `prev` (a scalar, or one value
    per stream) stands before x[..., 0] in FM.  FM: gain * angle of the exact product x[n] conj(x[n-1]); PM: gain * angle
    of x[n]; AM: gain * |x[n]|.  Returns (..., n) float64."""
    x = np.asarray(x).astype(np.complex128)
    gain = float(np.float32(gain))
    if mode == POLAR_FM:
        p = np.concatenate([np.broadcast_to(np.asarray(prev, np.complex128), x.shape[:-1])[..., None], x[..., :-1]], axis=-1)
        # the product's parts as sums of two exact float64 products of float32 values: one rounding each
        # (+ 0.0: a product that vanishes has the angle 0, whatever the signs of its zeros)
        return gain * np.arctan2(x.imag * p.real - x.real * p.imag + 0.0, x.real * p.real + x.imag * p.imag + 0.0)
    if mode == POLAR_PM:
        return gain * np.arctan2(x.imag, x.real)
    if mode == POLAR_AM:
        return gain * np.hypot(x.real, x.imag)
    raise ValueError("polar_reference: mode %r" % (mode,))


# ---- the spectrum occupancy detector (sfe_dsp_occ_*)
OCC_INFO = np.dtype([("floor", "<f4"), ("thr", "<f4"), ("count", "<u4"), ("status", "<u4")])
OCC_REC = np.dtype([("lo", "<i4"), ("hi", "<i4"), ("peak", "<i4"), ("peak_val", "<f4"), ("sum", "<f4"), ("moment", "<f4"),
                    ("zero", "<u4", (2,))])


def _occ_keys(v):
    """The total order of the law's step 3 as uint32: ascending keys are ascending float32 values, -0 below +0."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return b ^ np.where(b >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def _fma32(a, b, c):
    """fmaf(a, b, c) of float32 values whose product a b is exact in float64 (a is a small integer): the float64 sum is
    rounded to odd (its rounding error from TwoSum), so that the rounding to float32 is the only one that counts."""
    import math
    import struct
    p = float(a) * float(b)
    s = p + float(c)
    if math.isfinite(s):
        t = s - p
        err = (p - (s - t)) + (float(c) - t)
        if err != 0.0 and not struct.unpack("<q", struct.pack("<d", s))[0] & 1:
            s = math.nextafter(s, math.inf if err > 0 else -math.inf)
    return np.float32(s)


def occ_reference(rows, rank, factor, min_level=0.0, gap=0, min_width=1, max_emissions=16, shift=False):
    """The law of sfe_dsp_occ_* (include/sfe_dsp.h) restated in numpy on rows (..., N) float32: the floor by np.sort of the
    keys, the runs from the distances between occupied positions, the folds as explicit float32 operations.  Returns
    (info (rows,) OCC_INFO, rec (rows, max_emissions) OCC_REC, mask (rows, N) uint8)."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    x = x.reshape(1, -1) if x.ndim == 1 else x.reshape(-1, x.shape[-1])
    R, N = x.shape
    E, o = int(max_emissions), (N // 2 if shift else 0)
    info, rec, mask = np.zeros(R, OCC_INFO), np.zeros((R, E), OCC_REC), np.zeros((R, N), np.uint8)
    own = (np.arange(N) + N - o) % N                    # the row's own index of scan position p
    f32 = np.float32
    for i in range(R):
        xs = x[i, own]
        if not np.isfinite(xs).all():
            info[i] = (0, 0, 0, 1)
            info[i:i + 1].view(np.uint32)[:2] = 0x7FC00000
            continue
        keys = np.sort(_occ_keys(xs))
        k = keys[rank:rank + 1]
        floor = (k ^ np.where(k >> 31, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)[0]
        with np.errstate(over="ignore"):
            t = f32(factor) * floor
        m = f32(min_level)
        thr = t if _occ_keys(t)[()] >= _occ_keys(m)[()] else m
        at = np.flatnonzero(xs > thr)
        count = 0
        if at.size:
            cut = np.flatnonzero(np.diff(at) - 1 > gap)             # the gaps the closing leaves open
            los, his = at[np.r_[0, cut + 1]], at[np.r_[cut, at.size - 1]]
            wide = his - los + 1 >= min_width
            for lo, hi in zip(los[wide].tolist(), his[wide].tolist()):
                mask[i, own[lo:hi + 1]] = 1
                if count < E:
                    seg = xs[lo:hi + 1]
                    peak = lo + int(np.argmax(seg))                 # the first of equal maxima
                    total, moment = f32(0), f32(0)
                    for t0 in range(lo - lo % 16, hi + 1, 16):
                        ps, pm = f32(0), f32(0)
                        for p in range(max(lo, t0), min(hi, t0 + 15) + 1):
                            ps = ps + xs[p]
                            pm = _fma32(p - lo, xs[p], pm)
                        total, moment = total + ps, moment + pm
                    rec[i, count] = (lo - o, hi - o, peak - o, xs[peak], total, moment, (0, 0))
                count += 1
        info[i] = (floor, thr, count, 2 if count > E else 0)
    return info, rec, mask


# ---- the Reed-Solomon outer code (sfe_dsp_reed_*): an independent restatement.  The field multiply is shift-and-xor on numpy
# arrays (no table, nothing shared with the library); encoding is a polynomial remainder; decoding is
# Peterson-Gorenstein-Zierler -- linear algebra on the syndromes, no Berlekamp-Massey -- and every proposed correction is kept
# only if the corrected word's syndromes are all zero, so what it returns is a codeword within distance t or nothing.
def reed_gf_mul(a, b, prim):
    """a * b in GF(2^8) modulo the 9-bit polynomial prim, elementwise with broadcasting."""
    a, b = np.broadcast_arrays(np.asarray(a, np.uint32), np.asarray(b, np.uint32))
    a, r = a.copy(), np.zeros(a.shape, np.uint32)
    for i in range(8):
        r ^= np.where((b >> i) & 1, a, 0).astype(np.uint32)
        a = a << 1
        a ^= np.where(a & 0x100, np.uint32(prim), 0).astype(np.uint32)
    return r


def reed_gf_pow(a, e, prim):
    """a ** e elementwise, e a non-negative integer."""
    a = np.asarray(a, np.uint32)
    r = np.ones(a.shape, np.uint32)
    while e:
        if e & 1:
            r = reed_gf_mul(r, a, prim)
        a, e = reed_gf_mul(a, a, prim), e >> 1
    return r


_reed_tables = {}


def reed_tables(prim, fcr, step, n, n_par):
    """(the n_par roots alpha^(step (fcr + i)), the locators X_j = alpha^(step (n - 1 - j)) of the byte positions j < n,
    g(x) as coefficients from x^n_par down to x^0).  Kept per shape; the arrays are not to be written to."""
    key = (prim, fcr, step, n, n_par)
    if key not in _reed_tables:
        _reed_tables[key] = _reed_make_tables(*key)
    return _reed_tables[key]


def _reed_make_tables(prim, fcr, step, n, n_par):
    roots = np.array([reed_gf_pow(2, step * (fcr + i) % 255, prim) for i in range(n_par)], np.uint32)
    X = np.array([reed_gf_pow(2, step * (n - 1 - j) % 255, prim) for j in range(n)], np.uint32)
    g = np.array([1], np.uint32)
    for r in roots:
        g = np.concatenate([g, [0]]) ^ np.concatenate([[0], reed_gf_mul(g, r, prim)]).astype(np.uint32)
    return roots, X, g


def reed_syndromes(words, roots, prim):
    """words (m, n) -> (m, n_par): word(root_i), byte j the coefficient of x^(n - 1 - j)."""
    words = np.asarray(words, np.uint32)
    S = np.zeros((words.shape[0], roots.size), np.uint32)
    for j in range(words.shape[1]):
        S = reed_gf_mul(S, roots[None, :], prim) ^ words[:, j:j + 1]
    return S


def reed_encode_words(msgs, g, prim):
    """msgs (m, k) -> codewords (m, n): the message, then x^n_par m(x) mod g(x) by long division."""
    msgs = np.asarray(msgs, np.uint32)
    k, n_par = msgs.shape[1], g.size - 1
    work = np.concatenate([msgs, np.zeros((msgs.shape[0], n_par), np.uint32)], axis=1)
    for j in range(k):
        work[:, j:j + n_par + 1] ^= reed_gf_mul(work[:, j:j + 1].copy(), g[None, :], prim)
    return np.concatenate([msgs, work[:, k:]], axis=1)


def _reed_eliminate(A, b, prim):
    """Gaussian elimination of A x = b over the field: (rank of A, x where A is square and nonsingular, else None)."""
    A = np.concatenate([np.asarray(A, np.uint32), np.asarray(b, np.uint32).reshape(-1, 1)], axis=1)
    rows, cols = A.shape[0], A.shape[1] - 1
    rank = 0
    for c in range(cols):
        nz = np.flatnonzero(A[rank:, c]) if rank < rows else np.array([], int)
        if nz.size == 0:
            continue
        p = rank + int(nz[0])
        A[[rank, p]] = A[[p, rank]]
        A[rank] = reed_gf_mul(A[rank], reed_gf_pow(A[rank, c], 254, prim), prim)
        f = A[:, c].copy()
        f[rank] = 0
        A ^= reed_gf_mul(f[:, None], A[rank][None, :], prim)
        rank += 1
    return rank, (A[:, cols].copy() if rank == rows == cols else None)


def _reed_pgz(r, S, X, fcr, t, prim):
    """One received word r (n,) with syndromes S, not all zero: the error values per position (n,) of a proposal with at
    most t errors, or None."""
    S = S.astype(np.uint32)
    hankel = lambda e: np.array([[S[i + j] for j in range(e)] for i in range(e)], np.uint32)
    e, lam = _reed_eliminate(hankel(t), np.zeros(t, np.uint32), prim)[0], None
    while e >= 1:                                       # the largest e whose syndrome matrix is nonsingular
        _, sol = _reed_eliminate(hankel(e), S[e:2 * e], prim)       # sum_j S[i + j] Lambda_(e - j) = S[i + e]
        if sol is not None:
            lam = np.concatenate([[1], sol[::-1]]).astype(np.uint32)     # Lambda_0 .. Lambda_e
            break
        e -= 1
    if lam is None:
        return None
    z = reed_gf_pow(X, 254, prim)
    val = np.zeros(X.size, np.uint32)
    for c in lam[::-1]:
        val = reed_gf_mul(val, z, prim) ^ c
    at = np.flatnonzero(val == 0)                       # roots among the n positions of the code only
    if at.size != e:
        return None
    V = np.array([reed_gf_pow(X[at], i, prim) for i in range(e)], np.uint32)
    _, Y = _reed_eliminate(V, S[:e], prim)              # sum_k Y_k X_k^i = S_i, Y = value * X^fcr
    if Y is None:
        return None
    err = np.zeros(X.size, np.uint32)
    err[at] = reed_gf_mul(Y, reed_gf_pow(reed_gf_pow(X[at], fcr, prim), 254, prim), prim)
    return err


def reed_decode_words(words, prim, fcr, step, n_par, brute=False):
    """words (m, n) de-whitened received words -> (words corrected where a codeword lies within t, counts (m,): the distance,
    or -1 for an uncorrectable word, which stays as received).  brute (t = 1 only): instead of solving anything, try the word
    itself and every word at distance 1."""
    words = np.ascontiguousarray(words, np.uint8)
    m, n = words.shape
    t = n_par // 2
    roots, X, _ = reed_tables(prim, fcr, step, n, n_par)
    S = reed_syndromes(words, roots, prim)
    out, counts = words.copy(), np.full(m, -1, np.int64)
    counts[~S.any(axis=1)] = 0
    dirty = np.flatnonzero(S.any(axis=1))
    if brute:
        assert t == 1
        for w in dirty:
            cand = np.repeat(words[w:w + 1], n * 255, axis=0)
            cand[np.arange(n * 255), np.repeat(np.arange(n), 255)] ^= np.tile(np.arange(1, 256, dtype=np.uint8), n)
            ok = np.flatnonzero(~reed_syndromes(cand, roots, prim).any(axis=1))
            assert ok.size <= 1                         # minimum distance n_par + 1 >= 3
            if ok.size:
                out[w], counts[w] = cand[ok[0]], 1
        return out, counts
    tried = []
    for w in dirty:
        err = _reed_pgz(words[w], S[w], X, fcr, t, prim)
        if err is not None and 1 <= np.count_nonzero(err) <= t:
            tried.append((w, err.astype(np.uint8)))
    if tried:
        idx = np.array([w for w, _ in tried])
        cand = words[idx] ^ np.stack([e for _, e in tried])
        good = ~reed_syndromes(cand, roots, prim).any(axis=1)
        for (w, e), c, g in zip(tried, cand, good):
            if g:
                out[w], counts[w] = c, np.count_nonzero(e)
    return out, counts


def reed_reference(prim, fcr, step, n, n_par, depth, data, whiten=None, encode=False, status_in=None, brute=False):
    """The law of sfe_dsp_reed_* (include/sfe_dsp.h) restated in numpy, what api.reed_plan returns: with encode, payloads
    (n_frames, depth (n - n_par)) -> frames (n_frames, depth n); without, channel bytes (n_frames, depth n) -> (bytes, record
    (n_frames, 2) uint32, status (n_frames,) int32)."""
    d = np.asarray(data, np.uint8)
    d = d.reshape(1, -1) if d.ndim == 1 else d
    nf, k, I = d.shape[0], n - n_par, depth
    w = np.zeros(I * n, np.uint8) if whiten is None else np.asarray(whiten, np.uint8).ravel()
    if encode:
        _, _, g = reed_tables(prim, fcr, step, n, n_par)
        msgs = d[:, :I * k].reshape(nf, k, I).transpose(0, 2, 1).reshape(nf * I, k)      # codeword i of a frame: bytes j I + i
        code = reed_encode_words(msgs, g, prim).astype(np.uint8)
        return np.ascontiguousarray(code.reshape(nf, I, n).transpose(0, 2, 1).reshape(nf, I * n)) ^ w[None, :]
    up = np.zeros(nf, bool) if status_in is None else np.asarray(status_in).ravel() != 0
    words = (d[:, :I * n] ^ w[None, :]).reshape(nf, n, I).transpose(0, 2, 1).reshape(nf * I, n)
    fixed, counts = reed_decode_words(words, prim, fcr, step, n_par, brute=brute)
    out = np.ascontiguousarray(fixed.reshape(nf, I, n)[:, :, :k].transpose(0, 2, 1).reshape(nf, I * k))
    counts = counts.reshape(nf, I)
    rec = np.zeros((nf, 2), np.uint32)
    rec[:, 0] = np.where(counts > 0, counts, 0).sum(axis=1)
    rec[:, 1] = ((counts < 0) << np.arange(I)[None, :]).sum(axis=1)
    st = (rec[:, 1] != 0).astype(np.int32)
    out[up], rec[up], st[up] = 0, (0, (1 << I) - 1), 2
    return out, rec, st


# ---- the beamformer / stream-mixing bank (sfe_dsp_beam_*): weights are (M, B, S) complex64 ((B, S): one band)
def _beam_weights(W, V):
    W = np.asarray(W, dtype=np.complex64)
    W = W[None] if W.ndim == 2 else W
    if W.ndim != 3:
        raise ValueError("beam weights must be (n_beams, n_in) or (n_bands, n_beams, n_in)")
    if V is not None:
        V = np.asarray(V, dtype=np.complex64).reshape(W.shape)
    return np.ascontiguousarray(W), (None if V is None else np.ascontiguousarray(V))


def beam_real_matrix(W, V=None):
    """The host twin of sfe_dsp_beam_plan: the real matrices R_k, (M, 2B, 2S) float32.  Row 2b / 2b+1 is Re / Im of beam
    b, column 2s / 2s+1 is Re / Im of stream s; every entry is formed in float64 from the float32 weights and rounded
    once.  With V absent the entries are W's own floats up to sign."""
    W, V = _beam_weights(W, V)
    M, B, S = W.shape
    R = np.empty((M, 2 * B, 2 * S), dtype=np.float32)
    if V is None:
        R[:, 0::2, 0::2] = W.real
        R[:, 0::2, 1::2] = -W.imag
        R[:, 1::2, 0::2] = W.imag
        R[:, 1::2, 1::2] = W.real
    else:
        wr, wi = W.real.astype(np.float64), W.imag.astype(np.float64)
        vr, vi = V.real.astype(np.float64), V.imag.astype(np.float64)
        R[:, 0::2, 0::2] = wr + vr
        R[:, 0::2, 1::2] = -wi + vi
        R[:, 1::2, 0::2] = wi + vi
        R[:, 1::2, 1::2] = wr - vr
    return R


def beam_reference(x, W, V=None, dtype=np.float64):
    """The law of sfe_dsp_beam_* evaluated on the rounded real matrices: x is (S, M, n) complex ((S, n) for one band),
    the result (B, M, n) ((B, n)) complex128 -- or, with dtype=np.float32, complex64 from a float32 matrix product
    (numpy's own summation order: a yardstick, not the kernel's bits)."""
    R = beam_real_matrix(W, V)
    M, B2, S2 = R.shape
    x = np.asarray(x)
    one = x.ndim == 2
    z = np.ascontiguousarray(x.reshape(S2 // 2, M, -1).astype(np.complex128))
    X = np.empty((M, S2, z.shape[2]), dtype=dtype)
    X[:, 0::2] = z.real.transpose(1, 0, 2)
    X[:, 1::2] = z.imag.transpose(1, 0, 2)
    Y = np.matmul(R.astype(dtype), X)                               # (M, 2B, n)
    y = (Y[:, 0::2] + 1j * Y[:, 1::2]).transpose(1, 0, 2)
    y = y.astype(np.complex128 if dtype == np.float64 else np.complex64)
    return y[:, 0] if one else y


def beam_steering_weights(n_in, n_beams):
    """(n_beams, n_in) complex64: a uniform linear array of n_in elements at half-wavelength spacing, beam b steered to
    sin(theta_b) = -1 + (2 b + 1) / n_beams (a sine grid), each row scaled to unit gain in its own direction:
    W[b][s] = exp(-j pi s sin(theta_b)) / n_in."""
    u = -1.0 + (2.0 * np.arange(n_beams) + 1.0) / n_beams
    s = np.arange(n_in)
    return (np.exp(-1j * np.pi * u[:, None] * s[None, :]) / n_in).astype(np.complex64)


# ---- the spatial covariance estimator (sfe_dsp_cov_*): x is (S, M, n) complex ((S, n): one band)
def cov_columns(x, S, M):
    """The real columns u of the law: (M, 2S, n) float64, row 2s / 2s+1 the real / imaginary part of stream s."""
    z = np.asarray(x).reshape(S, M, -1).astype(np.complex128)
    U = np.empty((M, 2 * S, z.shape[2]))
    U[:, 0::2] = z.real.transpose(1, 0, 2)
    U[:, 1::2] = z.imag.transpose(1, 0, 2)
    return U


def cov_reference(x, S, M, A, scale):
    """The law of sfe_dsp_cov_* in float64: the rows that n instants complete, (M, n // A, 2S, 2S).  float64 sums in
    numpy's order: the yardstick of the values, not of the kernel's bits."""
    U = cov_columns(x, S, M)
    rows = U.shape[2] // A
    U = U[:, :, :rows * A].reshape(M, 2 * S, rows, A)
    return float(scale) * np.einsum("kira,kjra->krij", U, U)


def fma32(a, b, c):
    """fmaf(a, b, c) elementwise on float32 arrays (broadcast), correctly rounded: one rounding, of the exact a b + c.
    float32(float64(a) float64(b) + float64(c)) rounds twice and is wrong on ties.  Here the product is exact in float64
    (48 bits), TwoSum gives the float64 sum's rounding error, and a sum that is inexact with an even mantissa is stepped to
    its neighbour in the error's direction (round to odd): float64 carries more than two bits beyond float32, so the
    rounding to float32 that follows is the only one that counts."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c)))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = np.asarray(p + c)
        t = s - p
        err = (p - (s - t)) + (c - t)
        step = np.isfinite(s) & (err != 0.0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(step, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
        return s.astype(np.float32)[()]


def cov_group(A, T=64):
    """(T, C) of the covariance estimator's summation order: C the smallest power of two with C C >= A / T."""
    c = 1
    while c * c * T < A:
        c *= 2
    return T, c


def cov_law_reference(x, S, M, A, scale):
    """The law of sfe_dsp_cov_* in its own arithmetic, as include/sfe_dsp.h states the summation order: the rows that n
    instants complete, (M, n // A, 2S, 2S) float32, whose bits the device must give.  Per row: chunks of T = 64 instants,
    each the fma32 chain from +0 in ascending instant order; groups of C chunks (the last may be shorter), each the
    float32 left fold from 0 of its chunk partials; the row the float32 left fold from 0 of its group sums; then one
    float32 multiply by float32(scale).  x must hold float32 values.  Uses nothing of the library."""
    T, C = cov_group(A)
    U = cov_columns(x, S, M).astype(np.float32)
    rows, AC = U.shape[2] // A, A // T
    U = U[:, :, :rows * A].reshape(M, 2 * S, rows, A).transpose(0, 2, 1, 3)     # (M, rows, 2S, A): every row at once
    zero = np.zeros((M, rows, 2 * S, 2 * S), np.float32)
    total = zero
    for g in range(0, AC, C):
        group = zero
        for ch in range(g, min(g + C, AC)):
            part = zero
            for m in range(ch * T, (ch + 1) * T):
                part = fma32(U[:, :, :, None, m], U[:, :, None, :, m], part)
            group = group + part
        total = total + group
    return total * np.float32(scale)


def cov_from_gram(G):
    """(C, P) complex128 out of real Gram matrices (..., 2S, 2S): C = E[x x^H], the covariance, and P = E[x x^T], the
    pseudo-covariance."""
    G = np.asarray(G, dtype=np.float64)
    rr, ri, ir, ii = G[..., 0::2, 0::2], G[..., 0::2, 1::2], G[..., 1::2, 0::2], G[..., 1::2, 1::2]
    return (rr + ii) + 1j * (ir - ri), (rr - ii) + 1j * (ir + ri)


def mvdr_weights(C, steering, loading=0.0):
    """Minimum-variance distortionless-response weights in float64: w = R^-1 a / (a^H R^-1 a) with
    R = C + loading tr(C)/S I.  Returns the (1, 1, S) complex64 row w^H that Beam takes: y = w^H x has unit response on
    the steering vector a."""
    C = np.asarray(C, dtype=np.complex128)
    a = np.asarray(steering, dtype=np.complex128).ravel()
    S = a.size
    R = C.reshape(S, S) + loading * np.trace(C.reshape(S, S)).real / S * np.eye(S)
    Ra = np.linalg.solve(R, a)
    w = Ra / (a.conj() @ Ra)
    return w.conj().reshape(1, 1, S).astype(np.complex64)


def cov_scene(S, n, seed):
    """A uniform linear array of S elements at half-wavelength spacing (steering exp(j pi k sin theta)) that hears a
    unit-power QPSK signal d from 10 degrees, a complex normal interferer 30 dB above it from -35 degrees and, per
    element, complex normal noise 20 dB below it; the sum scaled to max |x| = 0.9.  Drawn from
    np.random.default_rng(seed) in that order.  Returns (x, x_d, x_i, a_d): the (S, n) complex64 sum, its desired and
    interferer parts (same scale, complex64) and the desired steering vector (complex128)."""
    rng = np.random.default_rng(seed)
    d = ((2.0 * rng.integers(0, 2, n) - 1.0) + 1j * (2.0 * rng.integers(0, 2, n) - 1.0)) / np.sqrt(2.0)
    i = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(10.0 ** 3.0 / 2.0)
    noise = (rng.standard_normal((S, n)) + 1j * rng.standard_normal((S, n))) * np.sqrt(10.0 ** -2.0 / 2.0)
    k = np.arange(S)
    a_d = np.exp(1j * np.pi * k * np.sin(np.deg2rad(10.0)))
    a_i = np.exp(1j * np.pi * k * np.sin(np.deg2rad(-35.0)))
    x_d, x_i = a_d[:, None] * d[None, :], a_i[:, None] * i[None, :]
    g = 0.9 / np.abs(x_d + x_i + noise).max()
    return ((g * (x_d + x_i + noise)).astype(np.complex64), (g * x_d).astype(np.complex64), (g * x_i).astype(np.complex64), a_d)


def mvdr_scene_rectilinear(S, n, seed):
    """cov_scene with the interferer replaced by sqrt(10^3) exp(0.7j) standard_normal(n): a real-valued interferer on a
    fixed phase, 30 dB above the signal, whose pseudo-covariance is not zero -- what the widely-linear solver can use and
    the linear one cannot.  Drawn from np.random.default_rng(seed) in cov_scene's order (signal, interferer, noise).
    Returns (x, x_d, x_i, a_d) as cov_scene does."""
    rng = np.random.default_rng(seed)
    d = ((2.0 * rng.integers(0, 2, n) - 1.0) + 1j * (2.0 * rng.integers(0, 2, n) - 1.0)) / np.sqrt(2.0)
    i = np.sqrt(10.0 ** 3.0) * np.exp(0.7j) * rng.standard_normal(n)
    noise = (rng.standard_normal((S, n)) + 1j * rng.standard_normal((S, n))) * np.sqrt(10.0 ** -2.0 / 2.0)
    k = np.arange(S)
    a_d = np.exp(1j * np.pi * k * np.sin(np.deg2rad(10.0)))
    a_i = np.exp(1j * np.pi * k * np.sin(np.deg2rad(-35.0)))
    x_d, x_i = a_d[:, None] * d[None, :], a_i[:, None] * i[None, :]
    g = 0.9 / np.abs(x_d + x_i + noise).max()
    return ((g * (x_d + x_i + noise)).astype(np.complex64), (g * x_d).astype(np.complex64), (g * x_i).astype(np.complex64), a_d)


def mvdr_loaded_matrix(G, widely_linear=False, load_rel=0.0, load_abs=0.0, dtype=np.float64):
    """Steps 1-3 of the law of sfe_dsp_mvdr_* on one Gram matrix (2S, 2S): the upper triangle mirrored, the mode's
    structure, the diagonal loading; in `dtype`."""
    G = np.asarray(G).astype(dtype)
    G = np.triu(G) + np.triu(G, 1).T
    if not widely_linear:
        h = (G[0::2, 0::2] + G[1::2, 1::2]) / dtype(2)
        x = (G[1::2, 0::2] - G[0::2, 1::2]) / dtype(2)
        G = np.empty_like(G)
        G[0::2, 0::2], G[1::2, 1::2], G[1::2, 0::2], G[0::2, 1::2] = h, h, x, -x
    n = G.shape[0]
    lam = dtype(load_abs) + dtype(load_rel) * np.trace(G) / dtype(n)
    return G + lam * np.eye(n, dtype=dtype)


def mvdr_rhs(a, dtype=np.float64):
    """A2 = [u(a), u(ja)], (2S, 2), of one steering vector."""
    a = np.asarray(a, dtype=np.complex128).ravel()
    A2 = np.empty((2 * a.size, 2), dtype=dtype)
    A2[0::2, 0], A2[1::2, 0], A2[0::2, 1], A2[1::2, 1] = a.real, a.imag, -a.imag, a.real
    return A2


def mvdr_fallback(steering):
    """The conventional beamformer W = conj(a) / |a|^2, V = 0 of every steering vector as Beam's real matrices,
    (M, 2B, 2S) float64 ((B, S) steering is one band)."""
    a = np.asarray(steering, dtype=np.complex64).astype(np.complex128)
    a = a[None] if a.ndim == 2 else a
    W = a.conj() / (np.abs(a) ** 2).sum(axis=2, keepdims=True)
    R = np.empty((a.shape[0], 2 * a.shape[1], 2 * a.shape[2]))
    R[:, 0::2, 0::2], R[:, 0::2, 1::2], R[:, 1::2, 0::2], R[:, 1::2, 1::2] = W.real, -W.imag, W.imag, W.real
    return R


def mvdr_reference(G, steering, widely_linear=False, load_rel=0.0, load_abs=0.0):
    """The law of sfe_dsp_mvdr_* in float64 numpy, independent of the C code: G is (M, 2S, 2S) ((2S, 2S): one band),
    steering (M, B, S) ((B, S)) complex, taken at complex64.  Returns (R (M, 2B, 2S), power (M, B), status (M,)) in
    float64 / int: a failed beam holds the fallback rows and a NaN power."""
    a = np.asarray(steering, dtype=np.complex64).astype(np.complex128)
    a = a[None] if a.ndim == 2 else a
    M, B, S = a.shape
    G = np.asarray(G, dtype=np.float64).reshape(M, 2 * S, 2 * S)
    R, power, status = mvdr_fallback(a), np.full((M, B), np.nan), np.zeros(M, dtype=np.int32)
    for k in range(M):
        Gh = mvdr_loaded_matrix(G[k], widely_linear, load_rel, load_abs)
        try:
            if not np.isfinite(Gh).all():
                raise np.linalg.LinAlgError
            L = np.linalg.cholesky(Gh)
        except np.linalg.LinAlgError:
            status[k] = 1
            continue
        for b in range(B):
            A2 = mvdr_rhs(a[k, b])
            if widely_linear and S == 1:        # A2 is square: R = A2^-1 (the fallback's own value), Q^-1 = A2^-1 G^ A2^-T
                power[k, b] = np.trace(Gh) / (np.abs(a[k, b, 0]) ** 2)
                continue
            Z = np.linalg.solve(L.T, np.linalg.solve(L, A2))
            if widely_linear:
                Q = A2.T @ Z
                q00, q01, q11 = Q[0, 0], Q[0, 1], Q[1, 1]
                det = q00 * q11 - q01 * q01
                if not (np.isfinite(det) and det > 0):
                    status[k] = 2
                    continue
                R[k, 2 * b] = (q11 * Z[:, 0] - q01 * Z[:, 1]) / det
                R[k, 2 * b + 1] = (q00 * Z[:, 1] - q01 * Z[:, 0]) / det
                power[k, b] = (q00 + q11) / det
            else:
                q = A2[:, 0] @ Z[:, 0]
                if not (np.isfinite(q) and q > 0):
                    status[k] = 2
                    continue
                r = Z[:, 0] / q
                R[k, 2 * b] = r
                R[k, 2 * b + 1, 0::2], R[k, 2 * b + 1, 1::2] = -r[1::2], r[0::2]
                power[k, b] = 2.0 / q
    return R, power, status


def eig_reference(G, steering, widely_linear=False, signal_dim=0, n_vec=0):
    """The law of sfe_dsp_eig_* in float64 numpy (numpy.linalg.eigh), independent of the C code: G is (M, 2S, 2S)
    ((2S, 2S): one band), steering (M, B, S) ((B, S)) complex, taken at complex64, or None (no beams).  Returns
    (values (M, 2S), null (M, B), vectors (M, 2 n_vec, 2S), status (M,), V (M, 2S, 2S)): V holds every eigenvector as a
    column, in the order of the values, signed by the law's rule.  A failed problem (a non-finite G^) holds NaN values
    and null spectrum and the selection matrix."""
    G = np.asarray(G, dtype=np.float64)
    G = G[None] if G.ndim == 2 else G
    M, n = G.shape[0], G.shape[1]
    S, E, D = n // 2, int(n_vec), int(signal_dim)
    if steering is None:
        a = np.zeros((M, 0, S), np.complex128)
    else:
        a = np.asarray(steering, dtype=np.complex64).astype(np.complex128)
        a = a[None] if a.ndim == 2 else a
    B = a.shape[1]
    values, null, status = np.full((M, n), np.nan), np.full((M, B), np.nan), np.zeros(M, dtype=np.int32)
    vectors, Vall = np.tile(np.eye(2 * E, n), (M, 1, 1)), np.tile(np.eye(n), (M, 1, 1))
    for k in range(M):
        with np.errstate(invalid="ignore", over="ignore"):
            Gh = mvdr_loaded_matrix(G[k], widely_linear)
        if not np.isfinite(Gh.astype(np.float32)).all():
            status[k] = 1
            continue
        lam, V = np.linalg.eigh(Gh)
        lam, V = lam[::-1], V[:, ::-1]
        lead = np.abs(V).argmax(axis=0)
        V = V * np.where(V[lead, np.arange(n)] < 0, -1.0, 1.0)[None, :]
        values[k], Vall[k] = lam, V
        if widely_linear:
            vectors[k] = V[:, :2 * E].T
        else:
            r = V[:, 0:2 * E:2].T
            vectors[k, 0::2] = r
            vectors[k, 1::2, 0::2], vectors[k, 1::2, 1::2] = -r[:, 1::2], r[:, 0::2]
        N = V[:, D:]
        for b in range(B):
            P = N.T @ mvdr_rhs(a[k, b])
            q00, q11, q01 = P[:, 0] @ P[:, 0], P[:, 1] @ P[:, 1], P[:, 0] @ P[:, 1]
            lmin = 0.5 * (q00 + q11) - np.hypot(0.5 * (q00 - q11), q01)
            null[k, b] = max(lmin, 0.0) / (np.abs(a[k, b]) ** 2).sum()
    return values, null, vectors, status, Vall


def offset_bytes(n_samples, bias=0, seed=SEED):
    """2 n uint8 (I,Q) bytes, uniformly random: over all 256 values with bias = 0 (the converted stream has a mean near 0),
    or over [2 bias, 256) (a mean near 128 + bias: bias = 38 gives bytes around 166, a converted mean near 0.3)."""
    rng = np.random.default_rng(seed)
    return rng.integers(2 * int(bias), 256, size=2 * int(n_samples), dtype=np.uint8)


def u8_to_cf32(b):
    """The receive converter's law (sfe_dsp_rx_u8_to_f32) in float32: (b - 128) * (1/127)."""
    return ((np.asarray(b, dtype=np.uint8).astype(np.float32) - np.float32(128.0)) * np.float32(1.0 / 127.0)).view(np.complex64)


# ---- the burst demodulator (sfe_dsp_burst_*): a pulse-shaped PSK burst whose timing, carrier and amplitude are known exactly
def raised_cosine(t, beta=0.35):
    """The raised-cosine pulse at times t (in symbols), float64: 1 at 0, 0 at every other integer."""
    t = np.asarray(t, dtype=np.float64)
    den = 1.0 - (2.0 * beta * t) ** 2
    edge = np.abs(den) < 1e-12
    h = np.sinc(t) * np.cos(np.pi * beta * t) / np.where(edge, 1.0, den)
    return np.where(edge, (np.pi / 4.0) * np.sinc(1.0 / (2.0 * beta)), h)


def psk_symbols(n, order=4, seed=SEED):
    """n unit-modulus symbols, float64: BPSK (order 2: +-1) or QPSK (order 4: the odd multiples of pi/4)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, order, size=int(n))
    return np.exp(1j * (2.0 * np.pi * k / order + (np.pi / 4.0 if order == 4 else 0.0)))


def burst_signal(symbols, sps, n, start, tau=0.0, f=0.0, phase=0.0, amp=1.0, beta=0.35, span=32):
    """n complex64 samples holding one burst: symbol k of `symbols` peaks at sample start + k sps + tau (tau in samples,
    any real number: the pulse is evaluated analytically at the shifted times), shaped by a raised cosine of roll-off
    beta cut at +-span symbols, then turned by a carrier of f turns per symbol whose phase is `phase` radians at symbol
    0, and scaled by amp.  No noise.  Computed in float64, rounded once."""
    a = np.asarray(symbols, dtype=np.complex128)
    t = (np.arange(int(n), dtype=np.float64) - start - tau) / sps        # in symbols, 0 at symbol 0's peak
    k0 = np.floor(t).astype(np.int64)
    x = np.zeros(int(n), np.complex128)
    for d in range(-span, span + 2):
        k = k0 + d
        ok = (k >= 0) & (k < a.size)
        x[ok] += a[k[ok]] * raised_cosine(t[ok] - k[ok], beta)
    return (amp * x * np.exp(1j * (2.0 * np.pi * f * t + phase))).astype(np.complex64)


def burst_cases(sps, n_sym, lag, seed=SEED):
    """The bursts the burst demodulator's tests and DESIGN.md 4.16 measure: per true tau in {-0.49 sps, -1.25, 0, 0.5,
    +0.49 sps} samples and true f in {0, +-0.02, 0.4 / lag} turns per symbol, (x complex64, o, the n_sym transmitted
    symbols, tau, f, phase, amp): an isolated burst whose symbol 0 peaks at sample o + tau of x.  QPSK and BPSK by turns
    (one sequence of each, drawn from `seed`); phase and amplitude differ from case to case."""
    out = []
    o, n = 3 * sps + 5, (n_sym + 8) * sps + 11
    for i, tau in enumerate((-0.49 * sps, -1.25, 0.0, 0.5, 0.49 * sps)):
        for j, f in enumerate((0.0, 0.02, -0.02, 0.4 / lag)):
            c = 4 * i + j
            a = psk_symbols(n_sym, 2 if c & 1 else 4, seed=seed)
            phase, amp = 0.7 * c - 2.9, 0.25 + 0.125 * c
            out.append((burst_signal(a, sps, n, o, tau, f, phase, amp), o, a, tau, f, phase, amp))
    return out


# ---- the Viterbi decoder (sfe_dsp_vit_*): payloads, the channel's soft values, and coded bits as symbols
def vit_bits(n, seed=SEED):
    """n payload bits (uint8 0 / 1) drawn from `seed`."""
    return np.random.default_rng(seed).integers(0, 2, size=int(n)).astype(np.uint8)


def vit_pack(bits):
    """Bits packed MSB-first into bytes, pad bits 0: what the decoder writes for them."""
    return np.packbits(np.asarray(bits, dtype=np.uint8))


def vit_soft(coded, ebn0_db=None, rate=0.5, seed=SEED):
    """The soft values of coded bits sent as BPSK, float32: 1 - 2c, plus -- with ebn0_db -- white Gaussian noise of
    variance 1 / (2 rate Eb/N0) drawn from `seed`.  A positive value favours bit 0."""
    r = 1.0 - 2.0 * np.asarray(coded, dtype=np.float64)
    if ebn0_db is not None:
        sigma = np.sqrt(1.0 / (2.0 * rate * 10.0 ** (ebn0_db / 10.0)))
        r = r + sigma * np.random.default_rng(seed).standard_normal(r.shape)
    return r.astype(np.float32)


def vit_symbols(coded, order=2):
    """Coded bits as unit-modulus symbols, complex128: BPSK (order 2: 1 - 2c) or Gray QPSK (order 4: bits 2i and 2i+1 on
    the real and the imaginary part, each (1 - 2c) / sqrt 2; an odd count is padded with a 0 bit)."""
    c = np.asarray(coded, dtype=np.float64).ravel()
    if order == 2:
        return (1.0 - 2.0 * c).astype(np.complex128)
    if c.size & 1:
        c = np.concatenate([c, [0.0]])
    return ((1.0 - 2.0 * c[0::2]) + 1j * (1.0 - 2.0 * c[1::2])) / np.sqrt(2.0)


# ---- the burst modulator (sfe_dsp_mod_*): the law restated in numpy, and the transmit wire format on the host
def mod_symbols(coded, order, amp, preamble=None):
    """The N symbols of one burst as complex64, float32 components exactly as the law forms them: amp * p[k] (one float32
    product per component) for the preamble, then the coded bits as BPSK (amp (1 - 2c), +0) or Gray QPSK (float32(amp /
    sqrt 2) per component, an odd count padded with a 0 bit)."""
    amp = np.float32(amp)
    c = np.asarray(coded, dtype=np.uint8).ravel()
    if order == 2:
        re, im = np.where(c == 1, -amp, amp).astype(np.float32), np.zeros(c.size, np.float32)
    else:
        if c.size & 1:
            c = np.concatenate([c, np.zeros(1, np.uint8)])
        a4 = np.float32(np.float64(amp) / np.sqrt(np.float64(2.0)))
        re, im = np.where(c[0::2] == 1, -a4, a4).astype(np.float32), np.where(c[1::2] == 1, -a4, a4).astype(np.float32)
    s = np.empty(re.size, np.complex64)
    s.real, s.imag = re, im
    if preamble is None or len(preamble) == 0:
        return s
    p = np.asarray(preamble, dtype=np.complex64).ravel()
    ps = np.empty(p.size, np.complex64)
    ps.real, ps.imag = amp * p.real, amp * p.imag
    return np.concatenate([ps, s])


def mod_reference(symbols, taps, sps, absolute=False):
    """The modulator's waveform law in float64: frame sample k sps + r = sum over q of h[q sps + r] s[k - q], h zero from
    n_taps on, s zero outside [0, N) -- the (N + Q - 1) sps samples of one frame as complex128.  absolute: the same sum
    on |h| and on |Re s|, |Im s| (the A of the direct-sum error bound)."""
    s = np.asarray(symbols).astype(np.complex128).ravel()
    h = np.asarray(taps, dtype=np.float32).astype(np.float64).ravel()
    sps = int(sps)
    Q = -(-h.size // sps)
    hp = np.concatenate([h, np.zeros(Q * sps - h.size)])
    if absolute:
        s, hp = np.abs(s.real) + 1j * np.abs(s.imag), np.abs(hp)
    y = np.zeros((s.size + Q - 1, sps), np.complex128)
    for q in range(Q):                                  # arm r of row k gets h[q sps + r] s[k - q]
        y[q:q + s.size, :] += s[:, None] * hp[None, q * sps:(q + 1) * sps]
    return y.ravel()


def tx10_pack(x):
    """The transmit converter's law (sfe_dsp_tx_f32_to_10bit) on the host: float32 values, four to a 5-byte group, each
    ((short)(x * 511) + 512) & 0x3FF -- the high two bits of the four in byte 0, the low bytes behind it."""
    x = np.ascontiguousarray(x).view(np.float32).ravel()
    u = ((x * np.float32(511)).astype(np.int32).astype(np.int16).astype(np.int32) + 512) & 0x3FF
    u = u[:u.size // 4 * 4].reshape(-1, 4)
    out = np.empty((u.shape[0], 5), np.uint8)
    out[:, 0] = (u[:, 0] >> 8) | ((u[:, 1] >> 8) << 2) | ((u[:, 2] >> 8) << 4) | ((u[:, 3] >> 8) << 6)
    out[:, 1:] = u & 0xFF
    return out.ravel()


def tx10_unpack(b):
    """The values a receiver of the transmit wire format sees, float32: (u - 512) / 511 of each 10-bit word."""
    b = np.asarray(b, dtype=np.uint8).reshape(-1, 5).astype(np.int32)
    hi = np.stack([(b[:, 0] >> (2 * i)) & 3 for i in range(4)], axis=1)
    return ((((hi << 8) | b[:, 1:]) - 512).astype(np.float32) / np.float32(511)).ravel()


def f32_to_u8(x):
    """float32 values requantised to the receive wire format: the byte nearest to 127 x + 128, clipped to [0, 255]."""
    x = np.ascontiguousarray(x).view(np.float32).ravel().astype(np.float64)
    return np.clip(np.rint(x * 127.0 + 128.0), 0, 255).astype(np.uint8)


# ---- the quasi-cyclic LDPC code (sfe_dsp_ldpc_*): the law of include/sfe_dsp.h restated on the expanded matrix.  Nothing
# below knows of circulants or layers: H is a list of rows, each the ascending column indices of its ones.
def ldpc_expand(shift, Z):
    """The rows of H, row r Z + i at that index: the ascending columns c Z + (i + shift[r][c]) mod Z of its ones."""
    s = np.asarray(shift, dtype=np.int64)
    Z = int(Z)
    rows = []
    for r in range(s.shape[0]):
        cs = np.flatnonzero(s[r] >= 0)
        for i in range(Z):
            rows.append(np.sort(cs * Z + (i + s[r, cs]) % Z))
    return rows


def ldpc_dense(rows, n):
    """H as (m, n) uint8."""
    H = np.zeros((len(rows), int(n)), np.uint8)
    for r, cols in enumerate(rows):
        H[r, cols] = 1
    return H


def gf2_solve(B, S):
    """X with B X = S over GF(2) -- B (m, m), S (m, w), entries 0 / 1 -- or None where B is singular: Gauss-Jordan on
    packed rows."""
    B, S = np.asarray(B, np.uint8), np.asarray(S, np.uint8)
    m = B.shape[0]
    M = np.packbits(np.concatenate([B, S], axis=1), axis=1)
    for p in range(m):
        byte, mask = p >> 3, 0x80 >> (p & 7)
        below = np.flatnonzero(M[p:, byte] & mask)
        if below.size == 0:
            return None
        if below[0]:
            M[[p, p + below[0]]] = M[[p + below[0], p]]
        col = M[:, byte] & mask
        col[p] = 0
        idx = np.flatnonzero(col)
        if idx.size:
            M[idx] ^= M[p]
    return np.unpackbits(M, axis=1)[:, m:m + S.shape[1]]


def ldpc_encodable(shift, Z):
    """Whether the last m columns of H are invertible over GF(2)."""
    s = np.asarray(shift)
    rows = ldpc_expand(s, Z)
    n = s.shape[1] * int(Z)
    H = ldpc_dense(rows, n)
    return gf2_solve(H[:, n - len(rows):], np.zeros((len(rows), 0), np.uint8)) is not None


def ldpc_encode_reference(shift, Z, data):
    """data (n_words, >= ceil(k / 8)) uint8, MSB-first: the codewords (n_words, ceil(n / 8)) uint8 with c[0 .. k) the payload
    and H c = 0, by solving B p = A u for all the words at once.  ValueError where the code is not encodable."""
    s = np.asarray(shift)
    rows = ldpc_expand(s, Z)
    m, n = len(rows), s.shape[1] * int(Z)
    k = n - m
    d = np.asarray(data, np.uint8)
    d = d.reshape(1, -1) if d.ndim == 1 else d
    u = np.unpackbits(d, axis=1)[:, :k]
    syn = np.stack([u[:, cols[cols < k]].sum(axis=1) & 1 for cols in rows]).astype(np.uint8)       # (m, n_words)
    B = ldpc_dense(rows, n)[:, k:]
    p = gf2_solve(B, syn)
    if p is None:
        raise ValueError("ldpc: the parity part of H is singular")
    return np.packbits(np.concatenate([u, p.T], axis=1), axis=1)


def ldpc_quantise(r, scale):
    """clamp(rint(r * scale), -127, 127) with the product in float32 and ties to even; r finite."""
    with np.errstate(over="ignore"):
        p = np.asarray(r, np.float32) * np.float32(scale)
    return np.clip(np.rint(p), -127, 127).astype(np.int32)


def _ldpc_runs(rows, one_at_a_time):
    """The rows in their order, cut into runs: consecutive rows of one degree that share no variable commute, so a run is
    updated in one step -- found from the rows themselves.  one_at_a_time: every run is a single row."""
    runs, cur, seen = [], [], set()
    for cols in rows:
        c = set(cols.tolist())
        if cur and not one_at_a_time and len(cols) == len(cur[0]) and not (c & seen):
            cur.append(cols)
            seen |= c
        else:
            if cur:
                runs.append(np.stack(cur))
            cur, seen = [cols], c
    runs.append(np.stack(cur))
    return runs


def ldpc_reference(shift, Z, x, scale=8.0, a=12, beta=0, max_iter=32, status_in=None, one_at_a_time=False, with_peak=False):
    """The decoder's law on x (n_words, n) float32 soft values, row after row of the expanded H in the order r Z + i:
    returns (bytes (n_words, ceil(k / 8)) uint8, record (n_words, 3) uint32, status (n_words,) int32), and with with_peak
    the largest |APP| met as a fourth item."""
    s = np.asarray(shift)
    rows = ldpc_expand(s, Z)
    m, n = len(rows), s.shape[1] * int(Z)
    k = n - m
    x = np.asarray(x, np.float32)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    W = x.shape[0]
    status = np.zeros(W, np.int32)
    status[~np.isfinite(x[:, :n]).all(axis=1)] = 1
    if status_in is not None:
        status[np.asarray(status_in).ravel() != 0] = 2
    ok = status == 0
    L = np.zeros((W, n), np.int32)
    L[ok] = ldpc_quantise(x[ok, :n], scale)
    runs = _ldpc_runs(rows, one_at_a_time)
    app = L.copy()
    msgs = [np.zeros((W,) + run.shape, np.int32) for run in runs]
    iters, unsat = np.zeros(W, np.uint32), np.zeros(W, np.uint32)
    peak = 0

    def unsatisfied(A):
        neg = A < 0
        return sum((neg[:, run].sum(axis=2) & 1).sum(axis=1) for run in runs).astype(np.uint32)

    act = np.flatnonzero(ok)
    unsat[act] = unsatisfied(app[act])
    act = act[unsat[act] != 0]
    for it in range(1, int(max_iter) + 1):
        if act.size == 0:
            break
        A = app[act]
        for run, R in zip(runs, msgs):
            d = run.shape[1]
            Q = A[:, run] - R[act]
            neg = Q < 0
            mag = np.abs(Q)
            js = mag.argmin(axis=2)                     # the lowest index among equals
            first = np.arange(d)[None, None, :] == js[:, :, None]
            m1 = mag.min(axis=2)
            m2 = np.where(first, 1 << 20, mag).min(axis=2)
            M = np.where(first, m2[:, :, None], m1[:, :, None])
            Mp = np.clip(((M * int(a)) >> 4) - int(beta), 0, 127)
            S = (neg.sum(axis=2) & 1).astype(bool)
            Rn = np.where(S[:, :, None] ^ neg, -Mp, Mp)
            A[:, run] = Q + Rn
            R[act] = Rn
        app[act] = A
        peak = max(peak, int(np.abs(A).max()))
        iters[act] = it
        unsat[act] = unsatisfied(A)
        act = act[unsat[act] != 0]
    status[ok & (unsat != 0)] = 3
    hard = (app < 0).astype(np.uint8)
    by = np.packbits(hard[:, :k], axis=1)
    flips = ((L != 0) & ((app < 0) != (L < 0))).sum(axis=1).astype(np.uint32)
    rec = np.stack([iters, unsat, flips], axis=1).astype(np.uint32)
    by[~ok], rec[~ok] = 0, 0
    out = (np.ascontiguousarray(by), np.ascontiguousarray(rec), status)
    return out + (peak,) if with_peak else out


# ---- the OFDM burst receiver (sfe_dsp_ofdm_*): a burst waveform made on the host, and the law restated in numpy
def ofdm_bins(kind):
    """(data bins, pilot bins) of a kind table, each in increasing k."""
    kind = np.asarray(kind, dtype=np.uint8).ravel()
    return np.flatnonzero(kind == 1), np.flatnonzero(kind == 2)


def ofdm_signal(n_fft, cp, n_train, kind, train, n, start, symbols=None, bits=None, pilot=None, pilot_sign=None, taps=(1.0,), eps=0.0,
                noise=0.0, seed=SEED):
    """n complex64 samples holding one OFDM burst from sample `start` on: n_train training symbols (train on the used
    bins) and the data symbols -- `symbols`, (n_data, Nd) complex on the data bins in increasing k, or `bits`, 2 n_data Nd
    coded bits as mod_symbols' Gray QPSK of unit modulus -- with pilot * pilot_sign[j] on the pilot bins, each an inverse
    transform with its cyclic prefix of cp samples; then the FIR channel `taps`, a frequency offset of eps subcarrier
    spacings counted from `start`, and complex Gaussian noise of standard deviation `noise` per component.  The transmit
    transform is scaled 1/N, so that H of the law is the channel's frequency response."""
    N = int(n_fft)
    data, pil = ofdm_bins(kind)
    if symbols is None:
        symbols = mod_symbols(bits, 4, 1.0).reshape(-1, data.size)
    symbols = np.asarray(symbols, dtype=np.complex128).reshape(-1, data.size)
    Ns = symbols.shape[0]
    sign = np.ones(Ns) if pilot_sign is None else np.asarray(pilot_sign, dtype=np.float64).ravel()
    train = np.asarray(train, dtype=np.complex128).ravel()
    X = np.zeros((n_train + Ns, N), np.complex128)
    used = np.concatenate([data, pil])
    X[:n_train, used] = train[used]
    X[n_train:, data] = symbols
    if pil.size and Ns:
        X[n_train:, pil] = np.asarray(pilot, dtype=np.complex128).ravel()[pil][None, :] * sign[:, None]
    t = np.fft.ifft(X, axis=1)
    frame = np.concatenate([t[:, N - cp:], t], axis=1).ravel()
    y = np.convolve(frame, np.asarray(taps, dtype=np.complex128))
    y = y * np.exp(2j * np.pi * float(eps) * np.arange(y.size) / N)
    out = np.zeros(int(n), np.complex128)
    hi = min(int(n), int(start) + y.size)
    out[int(start):hi] = y[:hi - int(start)]
    if noise:
        rng = np.random.default_rng(seed)
        out = out + float(noise) * (rng.standard_normal(out.size) + 1j * rng.standard_normal(out.size))
    return out.astype(np.complex64)


def ofdm_reference(x, o, n_fft, cp, advance, n_train, n_data, kind, train, pilot=None, pilot_sign=None, cfo_mode=0, cfo_skip=0, out_mode=0,
                   eps=None):
    """The law of sfe_dsp_ofdm_* on the burst that starts at sample o of the complex64 stream x, in float64 on np.fft,
    with the law's three hand-overs in float32 (eps, H, phi_j) and the table c rounded once: returns (symbols (n_data, Nd)
    complex64, chan (n_fft,) complex64, record (8,) float32, status).  Statuses 1 and 3 carry the law's bits; there is
    no gate here.  `eps`, where given with cfo_mode 1, is the float32 hand-over itself -- an implementation's own estimate,
    say -- and takes the place of angle(gamma) / 2 pi; everything behind the hand-over is the law's."""
    eps_in = eps
    N, L, T, Ns = int(n_fft), int(n_fft) + int(cp), int(n_train), int(n_data)
    data, pil = ofdm_bins(kind)
    used = np.concatenate([data, pil])
    x = np.asarray(x, dtype=np.complex64).ravel()

    def failed(st):
        rec = np.full(8, np.nan, np.float32)
        rec[6:] = 0.0
        return np.zeros((Ns, data.size), np.complex64), np.zeros(N, np.complex64), rec, st

    if o < 0 or o + (T + Ns) * L > x.size:
        return failed(3)
    r = x[o:o + (T + Ns) * L].astype(np.complex128).reshape(T + Ns, L)
    if not (np.isfinite(r.real).all() and np.isfinite(r.imag).all()):
        return failed(1)
    eps = np.float32(0.0)
    if cfo_mode:
        gamma = np.sum(r[:, cfo_skip + N:cp + N] * np.conj(r[:, cfo_skip:cp]))
        if gamma == 0 or not np.isfinite(gamma):
            return failed(1)
        eps = np.float32(np.angle(gamma) / (2.0 * np.pi)) if eps_in is None else np.float32(eps_in)
        nn = np.arange((T + Ns) * L, dtype=np.float64).reshape(T + Ns, L)
        turn = np.float64(eps) * nn / N
        r = r * np.exp(-2j * np.pi * (turn - np.rint(turn)))
    Y = np.fft.fft(r[:, cp - advance:cp - advance + N], axis=1)
    tr = np.asarray(train, dtype=np.complex64).ravel().astype(np.complex128)[used]
    c = (np.conj(tr) / (T * np.abs(tr) ** 2)).astype(np.complex64).astype(np.complex128)
    H = np.zeros(N, np.complex128)
    H[used] = (Y[:T, used].sum(axis=0) * c).astype(np.complex64)
    p = np.abs(H[used]) ** 2
    p32 = p.astype(np.float32)
    if not (np.all(p32 > 0) and np.isfinite(p32).all()):
        return failed(1)
    h2 = p.mean()
    sign = np.ones(Ns) if pilot_sign is None else np.asarray(pilot_sign, dtype=np.float64).ravel()
    phi = np.ones(Ns, np.complex128)
    D = Y[T:]
    perr = 0.0
    if pil.size and Ns:
        pl = np.asarray(pilot, dtype=np.complex64).ravel().astype(np.complex128)[pil]
        want = pl[None, :] * sign[:, None]
        P = np.sum(D[:, pil] * np.conj(H[pil][None, :] * want), axis=1)
        if np.any(P == 0) or not np.isfinite(P).all():
            return failed(1)
        phi = (P / np.abs(P)).astype(np.complex64).astype(np.complex128)
        zp = D[:, pil] * np.conj(H[pil][None, :] * phi[:, None]) / np.abs(H[pil][None, :]) ** 2
        perr = np.sum(np.abs(zp - want) ** 2) / (Ns * np.sum(np.abs(pl) ** 2))
    Z = D[:, data] * np.conj(H[data][None, :] * phi[:, None])
    Z = Z / (h2 if out_mode == 1 else np.abs(H[data][None, :]) ** 2)
    rec = np.array([eps, h2, p.min() / h2, perr, np.angle(phi[0]) / (2 * np.pi), np.angle(phi[-1]) / (2 * np.pi), 0.0, 0.0], np.float32)
    return Z.astype(np.complex64), H.astype(np.complex64), rec, 0


# ---- the QAM mapper and soft demapper (sfe_dsp_qam_*)
def qam_axis_words(m):
    """(u, bits): the odd integers u(w) of the 2^m axis words w = (b_0 .. b_(m-1)), b_0 the most significant bit of w, by the
    law's recursion, and the words' bits (2^m, m)."""
    def A(bits):
        return 1 if not bits else 2 ** len(bits) - (1 - 2 * bits[0]) * A(bits[1:])
    bits = [[(w >> (m - 1 - c)) & 1 for c in range(m)] for w in range(1 << m)]
    return np.array([(1 - 2 * b[0]) * A(b[1:]) for b in bits], np.int64), np.array(bits, np.uint8)


def qam_levels(order, amp=1.0):
    """The level table of the law, float32 [2^m]: float32(amp u(w) / sqrt(K)), K = 1 for order 2, else 2 (order - 1) / 3,
    formed in float64 from the float32 amp and rounded once."""
    bps = {2: 1, 4: 2, 16: 4, 64: 6, 256: 8}[int(order)]
    m = 1 if bps == 1 else bps // 2
    K = 1 if order == 2 else 2 * (int(order) - 1) // 3
    u, _ = qam_axis_words(m)
    return (np.float64(np.float32(amp)) * u.astype(np.float64) / np.sqrt(np.float64(K))).astype(np.float32)


def qam_points(order, amp=1.0):
    """(points complex128 [M], bits uint8 [M, bps]): every point of the constellation, its components the float32 levels,
    and the bps bits it carries in the order of the symbol-bit positions (I-axis bits first)."""
    lev = qam_levels(order, amp).astype(np.float64)
    bps = {2: 1, 4: 2, 16: 4, 64: 6, 256: 8}[int(order)]
    m = 1 if bps == 1 else bps // 2
    _, ab = qam_axis_words(m)
    if bps == 1:
        return lev.astype(np.complex128), ab
    wi, wq = np.divmod(np.arange(1 << bps), 1 << m)
    return lev[wi] + 1j * lev[wq], np.concatenate([ab[wi], ab[wq]], axis=1)


def qam_reference(sym, order, amp=1.0, scale=1.0, perm=None, csi=None, csi_index=None):
    """The max-log soft values of sfe_dsp_qam_* in float64, by brute force over all M points of the constellation and with
    no per-axis shortcut: for symbol z of a row and each of its bps bits, D0 and D1 are the least |z - p|^2 over the points p
    whose bit is 0 and 1, r = w (D1 - D0), w = scale, or scale |h|^2 with h = csi[row, csi_index[q mod len(csi_index)]].
    The float at perm[t] is symbol-bit position t's.  sym (n_rows, n_sym) complex; returns (n_rows, n_sym bps) float64."""
    z = np.atleast_2d(np.asarray(sym)).astype(np.complex128)
    pts, bits = qam_points(order, amp)
    bps = bits.shape[1]
    nr, ns = z.shape
    w = np.full((nr, ns), float(np.float32(scale)))
    if csi_index is not None:
        idx = np.asarray(csi_index, np.int64).ravel()
        h = np.atleast_2d(np.asarray(csi)).astype(np.complex128)[:, idx[np.arange(ns) % idx.size]]
        w = w * (h.real ** 2 + h.imag ** 2)
    out = np.empty((nr, ns, bps))
    step = max(1, (1 << 22) // pts.size)
    for r in range(nr):
        for a in range(0, ns, step):
            d = np.abs(z[r, a:a + step, None] - pts[None, :]) ** 2
            for c in range(bps):
                one = bits[:, c] == 1
                out[r, a:a + step, c] = w[r, a:a + step] * (d[:, one].min(axis=1) - d[:, ~one].min(axis=1))
    out = out.reshape(nr, ns * bps)
    if perm is not None:
        p = np.asarray(perm, np.int64).ravel()
        scattered = np.empty_like(out)
        scattered[:, p] = out
        out = scattered
    return out


# ------------------------------------------------------------------------------------------------ 2-(G)FSK (sfe_dsp_fsk_*)
def gfsk_pulse(bt, sps, span):
    """The GFSK frequency pulse: a Gaussian of bandwidth-time product bt convolved with a one-symbol rectangle, span * sps
    float32 taps centred on the span, normalised to sum 1 (float64 sum, rounded once per tap)."""
    import math
    n = int(span) * int(sps)
    t = (np.arange(n) - (n - 1) / 2.0) / float(sps)            # in symbols
    k = 2.0 * math.pi * float(bt) / math.sqrt(math.log(2.0))
    q = lambda v: 0.5 * math.erfc(v / math.sqrt(2.0))
    g = np.array([q(k * (v - 0.5)) - q(k * (v + 0.5)) for v in t], np.float64)
    return (g / g.sum()).astype(np.float32)


def fsk_delay(n_taps, n_mf):
    """The delay that centres a matched filter of n_mf taps on a symbol's pulse of n_taps (the discriminator's one sample
    included)."""
    return 1 + (int(n_taps) - int(n_mf)) // 2


def fsk_levels(pre, data_bits):
    """a = 1 - 2c over the preamble bits and the data bits, float64."""
    return 1.0 - 2.0 * np.concatenate([np.asarray(pre, np.float64).ravel(), np.asarray(data_bits, np.float64).ravel()])


def fsk_reference_mod(pre, data_bits, pulse, h, sps, amp=1.0):
    """One frame in float64, independent of the integer law: the phase in turns is a real-valued cumulative sum of h / 2 * a *
    g, the sample amp * exp(2 pi j phase).  F = (N + Q - 1) * sps + 1 samples, the first at phase 0."""
    a, g, sps = fsk_levels(pre, data_bits), np.asarray(pulse, np.float64).ravel(), int(sps)
    N, Q = a.size, -(-g.size // sps)
    F = (N + Q - 1) * sps + 1
    up = np.zeros(F - 1)
    up[:N * sps:sps] = a
    freq = np.convolve(up, g)[:F - 1] * (float(np.float32(h)) / 2.0)
    turns = np.concatenate([[0.0], np.cumsum(freq)])
    return float(np.float32(amp)) * np.exp(2j * np.pi * turns)


def fsk_expected(pre, pulse, sps, mf, delay):
    """e[k] of the preamble in float64 from the real-valued pulse (h cancels): the matched filter over the preamble's own
    frequency waveform, data symbols taken as 0, over (sum g / sps) * sum m."""
    a, g, m, sps = 1.0 - 2.0 * np.asarray(pre, np.float64).ravel(), np.asarray(pulse, np.float64).ravel(), np.asarray(mf, np.float64).ravel(), int(sps)
    Lp = a.size
    D = np.zeros((Lp - 1) * sps + g.size + int(delay) + Lp * sps + m.size)
    for k in range(Lp):
        D[k * sps:k * sps + g.size] += a[k] * g
    U = g.sum() / sps * m.sum()
    return np.array([np.dot(m, D[delay + k * sps - 1:][:m.size]) for k in range(Lp)]) / U


def fsk_reference_demod(x, o, pre, n_bits, pulse, sps, mf, delay, rng, scale=1.0):
    """One burst in float64: np.angle of x[n] conj(x[n-1]), dot products with the matched filter, the least-squares fit of
    (dev, dc) on the preamble at every timing candidate, the candidate of the greatest num (the lowest among equals).
    Returns (tau, f, dev, q, soft (n_bits,))."""
    x, m, sps, delay, R = np.asarray(x, np.complex128).ravel(), np.asarray(mf, np.float64).ravel(), int(sps), int(delay), int(rng)
    e = fsk_expected(pre, pulse, sps, mf, delay)
    Lp, N = e.size, e.size + int(n_bits)
    lo, hi = o + delay - R - 1, o + delay + R + (N - 1) * sps + m.size
    seg = x[lo:hi]
    v = np.angle(seg[1:] * np.conj(seg[:-1]))                   # v[i] of sample lo + 1 + i, i.e. relative index delay - R + i
    u = lambda tau, k: np.array([np.dot(m, v[R + tau + kk * sps:][:m.size]) for kk in k])
    se, see = e.sum(), (e * e).sum()
    den = Lp * see - se * se
    best = None
    for tau in range(-R, R + 1):
        uk = u(tau, range(Lp))
        S1, Se = uk.sum(), (e * uk).sum()
        num = Lp * Se - se * S1
        if best is None or num > best[0]:
            best = (num, tau, S1, uk)
    num, tau, S1, uk = best
    dev = num / den
    dc = (S1 - dev * se) / Lp
    q = ((uk - (dev * e + dc)) ** 2).sum() / (dev * dev * see)
    soft = float(np.float32(scale)) * (u(tau, range(Lp, N)) - dc) / dev
    return tau, dc / (2.0 * np.pi), dev, q, soft


# ------------------------------------------------------------------ frame check: CRC and scrambler (sfe_dsp_crc_*)
def pn_reference(m, taps, seed, n):
    """n bytes of the additive scrambler's sequence, bit by bit as include/sfe_dsp.h states it: a[i] = bit i of seed for
    i < m, a[k + m] = the xor of a[k + i] over the set bits i of taps; a[8 j] is bit 7 of byte j."""
    m, nbits = int(m), 8 * int(n)
    a = [(int(seed) >> i) & 1 for i in range(m)]
    at = [i for i in range(m) if (int(taps) >> i) & 1]
    for k in range(max(0, nbits - m)):
        v = 0
        for i in at:
            v ^= a[k + i]
        a.append(v)
    return np.packbits(np.array(a[:nbits], np.uint8))          # MSB first


def _crc_bits(width, poly, init, reflect, xorout, rows):
    """The CRC of every row of `rows` (n_frames, n) uint8, one shift of the register at a time, all frames at once."""
    w = int(width)
    nf = rows.shape[0]
    if w == 0:
        return np.zeros(nf, np.uint32)
    mask, top = np.uint64((1 << w) - 1), np.uint64(1 << (w - 1))
    r = np.full(nf, int(init), np.uint64)
    bits = np.unpackbits(rows, axis=1, bitorder="little" if reflect else "big")          # the order in which a byte's bits enter
    for j in range(bits.shape[1]):
        # a message bit enters at the register's top; a one leaving the top folds the polynomial in
        out = ((r & top) != 0) ^ (bits[:, j] != 0)
        r = (r << np.uint64(1)) & mask
        r[out] ^= np.uint64(int(poly))
    if reflect:
        rev = np.zeros(nf, np.uint64)
        for i in range(w):
            rev |= ((r >> np.uint64(i)) & np.uint64(1)) << np.uint64(w - 1 - i)
        r = rev
    return (r ^ np.uint64(int(xorout))).astype(np.uint32)


def crc_reference(width, poly, init, reflect, xorout, pn_m=0, pn_taps=0, pn_seed=0, payload_bytes=1, data=None, verify=False, status_in=None):
    """The law of sfe_dsp_crc_* (include/sfe_dsp.h) restated in numpy, what api.crc_plan returns: without verify, payloads
    (n_frames, P) -> frames (n_frames, P + width / 8); with verify, channel bytes (n_frames, Fb) -> (bytes, record (n_frames, 2)
    uint32, status (n_frames,) int32).  The register takes one message bit per shift (the bit-at-a-time form of the
    byte-at-a-time sentence), over all frames at once."""
    P, nt = int(payload_bytes), int(width) // 8
    Fb = P + nt
    d = np.asarray(data, np.uint8)
    d = d.reshape(1, -1) if d.ndim == 1 else d
    nf = d.shape[0]
    pn = pn_reference(pn_m, pn_taps, pn_seed, Fb) if pn_m else np.zeros(Fb, np.uint8)
    order = range(nt) if reflect else range(nt - 1, -1, -1)                             # the tail's bytes as shifts of the CRC
    if not verify:
        crc = _crc_bits(width, poly, init, reflect, xorout, d[:, :P])
        tail = np.stack([(crc >> np.uint32(8 * s)).astype(np.uint8) for s in order], axis=1) if nt else np.zeros((nf, 0), np.uint8)
        return np.concatenate([d[:, :P], tail], axis=1) ^ pn[None, :]
    r = d[:, :Fb] ^ pn[None, :]
    crc = _crc_bits(width, poly, init, reflect, xorout, r[:, :P])
    got = np.zeros(nf, np.uint32)
    for k, s in enumerate(order):
        got |= r[:, P + k].astype(np.uint32) << np.uint32(8 * s)
    by, rec = np.ascontiguousarray(r[:, :P]), np.stack([crc, got], axis=1).astype(np.uint32)
    st = (crc != got).astype(np.int32)
    if status_in is not None:
        up = np.asarray(status_in).ravel() != 0
        by[up], rec[up], st[up] = 0, 0, 2
    return by, rec, st
