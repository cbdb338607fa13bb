"""Every channelizer, combiner and down-converter kernel instantiation (csrc/chan.hip, combine.hip, ddc.hip) on the GPU
against the float64 references of their contracts (synth.chan_reference, combine_reference, ddc_reference and their
_direct forms).  `-m gpu`, except the two table checks at the end, which need no GPU.

One explicit case table per handle.  Every case runs with random asymmetric taps (a few keep the Hamming-sinc prototype,
for tone-like structure), with 2 or 3 streams at strides wider than the call: the input's padding holds NaN, and the
output's padding between rows and streams, and a guard band on both sides of it, hold a sentinel that must survive.  The
call is long enough to reach, by the tile rules restated below, a first tile that reads the carried history, an interior
tile (unguarded loads) and a partial last tile.  The same input fed to a fresh handle in a ragged list of calls (an odd
first call, a single output, calls shorter than the carried history) must give the one-call bits."""
import json
import os
import re

import numpy as np
import pytest

from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simplefe_amd", "csrc")
TOL = 1e-5
SENT = 0x7FC0DEAD           # a quiet-NaN pattern no kernel writes: every cf32 output padding word must keep it
SENT_TX10 = 0xA5A5A5A5      # the same for TX10 bytes
GUARD = 64                  # sentinel words before and after every output buffer

# (M, D, input format, n_taps, taps, n_streams): all 36 chan_kernel<log2 M, D != M, u8> instantiations.  The tap counts
# 8M - 3, 12M + 5, 16M + 1 (= 1 mod M) and 32M give every padded branch count (P rounded up to 8: 8, 16, 24, 32) at
# every M, rotated over (D, format) from one M to the next.
CHAN_CASES = [
    (4, 4, "cf32", 29, "rand", 2), (4, 2, "cf32", 53, "rand", 2), (4, 4, "u8", 65, "rand", 2), (4, 2, "u8", 128, "rand", 2),
    (8, 8, "cf32", 101, "rand", 3), (8, 4, "cf32", 129, "rand", 2), (8, 8, "u8", 256, "rand", 2), (8, 4, "u8", 61, "rand", 2),
    (16, 16, "cf32", 257, "lowpass", 2), (16, 8, "cf32", 512, "rand", 2), (16, 16, "u8", 125, "rand", 2),
    (16, 8, "u8", 197, "rand", 2),
    (32, 32, "cf32", 1024, "rand", 2), (32, 16, "cf32", 253, "rand", 3), (32, 32, "u8", 389, "rand", 2),
    (32, 16, "u8", 513, "rand", 2),
    (64, 64, "cf32", 509, "rand", 2), (64, 32, "cf32", 773, "rand", 2), (64, 64, "u8", 1025, "rand", 2),
    (64, 32, "u8", 2048, "lowpass", 2),
    (128, 128, "cf32", 1541, "rand", 2), (128, 64, "cf32", 2049, "rand", 2), (128, 128, "u8", 4096, "rand", 2),
    (128, 64, "u8", 1021, "rand", 3),
    (256, 256, "cf32", 4097, "rand", 2), (256, 128, "cf32", 8192, "lowpass", 2), (256, 256, "u8", 2045, "rand", 2),
    (256, 128, "u8", 3077, "rand", 2),
    (512, 512, "cf32", 16384, "rand", 2), (512, 256, "cf32", 4093, "rand", 2), (512, 512, "u8", 6149, "rand", 2),
    (512, 256, "u8", 8193, "rand", 2),
    (1024, 1024, "cf32", 8189, "rand", 2), (1024, 512, "cf32", 12293, "rand", 2), (1024, 1024, "u8", 16385, "lowpass", 2),
    (1024, 512, "u8", 32768, "rand", 2),
]

# (M, D, n_taps, taps, n_streams): all 63 combine_kernel<log2 M, D != M, log2 J> instantiations, J = P = ceil(L / D)
# rounded up to a power of two >= 8.  P sits just above a power of two (9, 17, 33) at every other M, at the top of its
# class (16, 32, 64) at the others; M = 1024 has L = 32M at both D (the two two-workgroup-per-instant shapes).
COMBINE_CASES = [
    (4, 4, 29, "rand", 3), (4, 4, 33, "rand", 2), (4, 4, 65, "rand", 2),
    (4, 2, 15, "rand", 2), (4, 2, 17, "rand", 2), (4, 2, 33, "rand", 2), (4, 2, 65, "rand", 2),
    (8, 8, 41, "rand", 2), (8, 8, 128, "rand", 2), (8, 8, 256, "rand", 2),
    (8, 4, 25, "rand", 2), (8, 4, 64, "rand", 2), (8, 4, 128, "rand", 2), (8, 4, 256, "rand", 2),
    (16, 16, 125, "rand", 2), (16, 16, 129, "rand", 2), (16, 16, 257, "rand", 2),
    (16, 8, 63, "rand", 2), (16, 8, 65, "lowpass", 2), (16, 8, 129, "rand", 3), (16, 8, 257, "rand", 2),
    (32, 32, 161, "rand", 2), (32, 32, 512, "rand", 2), (32, 32, 1024, "rand", 2),
    (32, 16, 97, "rand", 2), (32, 16, 256, "rand", 2), (32, 16, 512, "rand", 2), (32, 16, 1024, "rand", 2),
    (64, 64, 509, "rand", 2), (64, 64, 513, "rand", 2), (64, 64, 1025, "lowpass", 2),
    (64, 32, 255, "rand", 2), (64, 32, 257, "rand", 3), (64, 32, 513, "rand", 2), (64, 32, 1025, "rand", 2),
    (128, 128, 641, "rand", 2), (128, 128, 2048, "rand", 2), (128, 128, 4096, "rand", 2),
    (128, 64, 385, "rand", 2), (128, 64, 1024, "rand", 2), (128, 64, 2048, "rand", 2), (128, 64, 4096, "rand", 2),
    (256, 256, 2045, "lowpass", 2), (256, 256, 2049, "rand", 2), (256, 256, 4097, "rand", 2),
    (256, 128, 1023, "rand", 2), (256, 128, 1025, "rand", 2), (256, 128, 2049, "rand", 2), (256, 128, 4097, "lowpass", 2),
    (512, 512, 2561, "rand", 2), (512, 512, 8192, "rand", 2), (512, 512, 16384, "rand", 2),
    (512, 256, 1537, "rand", 2), (512, 256, 4096, "rand", 2), (512, 256, 8192, "rand", 2), (512, 256, 16384, "rand", 2),
    (1024, 1024, 8189, "rand", 2), (1024, 1024, 8193, "lowpass", 2), (1024, 1024, 32768, "rand", 2),
    (1024, 512, 4095, "rand", 2), (1024, 512, 8192, "rand", 2), (1024, 512, 8193, "rand", 2), (1024, 512, 32768, "rand", 2),
]

# (input format, D, K, n_taps, taps, n_streams): all 12 (format, tunings per chunk) pairs, each call with edge and
# interior tiles, so all 24 ddc_kernel<format, KT, T, guarded> instantiations.  K = 3 and 5, 9, 63 leave a chunk part
# filled; D runs along the lane-group boundaries; P = ceil(L / D) up to 64, and = 1 (mod 4) in several cases.
DDC_CASES = [
    ("cf32", 1, 1, 64, "rand", 2), ("cf32", 7, 2, 231, "rand", 3), ("cf32", 256, 3, 8192, "lowpass", 2),
    ("cf32", 1024, 4, 8192, "rand", 2), ("cf32", 1023, 8, 8192, "rand", 2), ("cf32", 2, 9, 128, "rand", 2),
    ("cf32", 257, 64, 3341, "rand", 2),
    ("u8", 2, 1, 34, "rand", 2), ("u8", 255, 2, 8192, "lowpass", 2), ("u8", 1, 4, 61, "rand", 3),
    ("u8", 7, 5, 448, "rand", 2), ("u8", 256, 8, 5117, "rand", 2), ("u8", 1024, 63, 5000, "rand", 2),
    ("real", 7, 1, 448, "rand", 2), ("real", 1024, 2, 5120, "lowpass", 2), ("real", 1, 3, 33, "rand", 2),
    ("real", 257, 4, 8000, "rand", 3), ("real", 255, 5, 5355, "rand", 2), ("real", 1023, 9, 4092, "rand", 2),
    ("real", 2, 64, 90, "rand", 2),
]
DDC_FORMATS = {"cf32": 0, "u8": 1, "real": 2}      # ddc.hip: DDC_CF32, DDC_U8, DDC_REAL


# The tile rules the call lengths come from, restated from the sources; test_tile_rules_follow_the_sources pins the
# lines they restate.  A layout lists a call's tiles in order: "h" reads the carried history, "i" is interior (every
# load unguarded), "e" is guarded at the call's end.

def _ceil(a, b):
    return -(-a // b)


def chan_layout(M, D, n_taps, n_out):
    """chan.hip, one call of n_out outputs: tiles of chan_tile_rows instants; a tile is interior when its first instant
    m has m D - (Ppad - 1) M - (M - 1) >= 0 (Ppad = P rounded up to CHAN_RU = 8) and it ends inside the call.
    Returns (instants per tile, tile kinds)."""
    rows = 16 * (256 // M) if M <= 256 else 8
    ppad = _ceil(_ceil(n_taps, M), 8) * 8
    return rows, ["h" if t * rows * D - ppad * M + 1 < 0 else "e" if (t + 1) * rows > n_out else "i"
                  for t in range(_ceil(n_out, rows))]


def chan_length(M, D, n_taps):
    """Outputs of a case's one call: through the first interior tile, then half a tile."""
    rows = chan_layout(M, D, n_taps, 1)[0]
    ppad = _ceil(_ceil(n_taps, M), 8) * 8
    return (max(1, _ceil(ppad * M - 1, rows * D)) + 1) * rows + rows // 2 + 1


def combine_layout(M, D, logj, n_in):
    """combine.hip / api_combine.hip, one call of n_in instants: a workgroup holds G = NT / (D / CS) segments of `run`
    instants and reads each in chunks of RG rows from W0 rows before it; a chunk loads unguarded when every row of the
    workgroup's G segments is an instant of the call.  run = 4 J rounded up to whole chunks, capped at n_in: the host's
    run while n_in n_streams <= 32 J G (8 workgroups per compute unit of G segments of 4 J instants, on any number of
    compute units).  Returns (G, run, tile kinds)."""
    logm = M.bit_length() - 1
    cs = 2 if logm == 10 and logj == (6 if D != M else 5) else 1
    G = max(256, D // cs) // (D // cs)
    rg = ((4096 >> logm if logm <= 8 else 8) >> (1 if logj == 6 else 0)) // G
    w0 = _ceil((1 << logj) - 1, rg) * rg
    run = _ceil(min(4 << logj, n_in), rg) * rg
    kinds = []
    for t in range(_ceil(n_in, G * run)):
        m00 = [m for m in (t * G * run - w0 + c * rg for c in range((w0 + run) // rg)) if m < n_in]
        kinds.append("h" if m00[0] < 0 else "i" if all(m + (G - 1) * run + rg <= n_in for m in m00) else "e")
    return G, run, kinds


def combine_length(M, D, logj):
    """Instants of a case's one call: two workgroups' runs and half of one more (the second workgroup is interior)."""
    G, run, _ = combine_layout(M, D, logj, 4 << logj)
    return 2 * G * run + G * run // 2 + 1


def ddc_tunings_per_chunk(K):
    return 1 if K == 1 else 2 if K == 2 else 4 if K <= 4 else 8


def ddc_layout(D, K, n_taps, n_out):
    """ddc.hip launch_ddc, one call of n_out outputs: tiles of G T instants (G = 256 / min(D, 256), T = 16 up to 2
    tunings per chunk, else 8); tiles [t_lo, t_hi) run the unguarded kernel, t_lo at the first instant m >= Ppad - 1
    (+1 for D > 1; Ppad = P rounded up to DDC_RU = 4).  Returns (instants per tile, tile kinds)."""
    rows = (256 // min(D, 256)) * (16 if ddc_tunings_per_chunk(K) <= 2 else 8)
    ppad = _ceil(_ceil(n_taps, D), 4) * 4
    tiles = _ceil(n_out, rows)
    t_lo = min(tiles, _ceil(ppad - 1 + (D > 1), rows))
    t_hi = max(t_lo, n_out // rows)
    return rows, ["h" if t < t_lo else "i" if t < t_hi else "e" for t in range(tiles)]


def ddc_length(D, K, n_taps):
    """Outputs of a case's one call: through the first interior tile, then half a tile."""
    rows = ddc_layout(D, K, n_taps, 1)[0]
    ppad = _ceil(_ceil(n_taps, D), 4) * 4
    return (max(1, _ceil(ppad - 1 + (D > 1), rows)) + 1) * rows + rows // 2 + 1


def _covered(kinds):
    return kinds[0] == "h" and "i" in kinds and kinds[-1] == "e"


def _cuts(n, hist):
    """A ragged split of n outputs (instants for the combiner) into calls: an odd first call, then a single output and
    calls shorter than the `hist` carried between calls, then two long calls."""
    first = (n // 3) | 1
    short = [1, 2, max(1, min(hist - 1, n // 6))]
    rest = n - first - sum(short)
    cuts = [first] + short + [rest // 2, rest - rest // 2]
    assert sum(cuts) == n and min(cuts) >= 1 and max(short) < hist, (n, hist, cuts)
    return cuts


# ------------------------------------------------------------------------------------------------------------------------
# device buffers and checks

@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


def _taps(kind, n_taps, cutoff, rng):
    if kind == "lowpass":
        return synth.lowpass_taps(n_taps, cutoff)
    return (rng.standard_normal(n_taps) / np.sqrt(n_taps)).astype(np.float32)


def _filled(api, n_words, word):
    """A device buffer of n_words 32-bit words and GUARD more on each side, every one holding `word`; returns (array,
    address of the first word past the front guard)."""
    d = api.DeviceArray.from_numpy(np.full(n_words + 2 * GUARD, word, np.uint32).view(np.float32))
    return d, d.ptr + 4 * GUARD


def _rows(d, word, n_rows, stride, used, dtype=np.uint32):
    """The n_rows rows of `stride` elements (dtype) after the front guard of _filled's buffer d: asserts that the
    guards, and every element of a row past `used`, still hold the fill; returns the (n_rows, used) elements."""
    w = d.to_numpy().view(dtype)
    fill = np.array([word], np.uint32).view(dtype)[0]
    g = 4 * GUARD // w.itemsize
    body = w[g:g + n_rows * stride].reshape(n_rows, stride)
    assert (w[:g] == fill).all() and (w[g + n_rows * stride:] == fill).all(), "a write outside the output rows"
    assert (body[:, used:] == fill).all(), "a write into the padding between rows"
    return body[:, :used].copy()


def _cf32(words):
    return words.view(np.float32).view(np.complex64)


def _padded(api, x, stride, fill):
    """x (rows, n) on the device as rows of `stride` elements, the rest `fill`."""
    a = np.full((x.shape[0], stride), fill, x.dtype)
    a[:, :x.shape[1]] = x
    return api.DeviceArray.from_numpy(a.view(np.float32))


def _u8_input(api, lib, b, offset):
    """Bytes b on the device `offset` bytes past a 16-byte boundary; returns (array, address of b[0])."""
    d = api.DeviceArray((b.size + offset) // 4 + 8)
    assert d.ptr % 16 == 0
    assert lib.sfe_dsp_memcpy_h2d(d.ptr + offset, b.ctypes.data, b.size, None) == 0
    return d, d.ptr + offset


def _u8_decode(b):
    """(I,Q) byte pairs as the device converts them, (b - 128) / 127 in float32, then float64 complex."""
    v = (b.astype(np.float32) - np.float32(128.0)) * np.float32(1.0 / 127.0)
    return v[..., 0::2].astype(np.float64) + 1j * v[..., 1::2].astype(np.float64)


def _check(got, ref, tag):
    """rel-RMS of every row (a channel, output phase or tuning) against the RMS of the reference's row."""
    err = got.astype(np.complex128) - ref
    rel = np.sqrt(np.mean(np.abs(err) ** 2, axis=-1) / np.mean(np.abs(ref) ** 2, axis=-1))
    assert rel.max() <= TOL, (tag, int(np.argmax(rel)), float(rel.max()))


def _chan_reference(x, h, M, D):
    # the FFT form runs M transforms as long as the call and the taps; for the wide banks the direct form's one matrix
    # product over the few instants of a call is far shorter
    if M * h.size >= 1 << 20:
        return synth.chan_reference_direct(x, h, M, D, 0, 0, x.size // D)
    return synth.chan_reference(x, h, M, D)


def _combine_reference(X, g, M, D):
    # the overlap-add form loops over the instants in Python: the direct form for the long calls of the narrow banks
    n = X.shape[1]
    if n > 4096:
        return synth.combine_reference_direct(X, g, M, D, 0, 0, n * D)
    return synth.combine_reference(X, g, M, D)


# ------------------------------------------------------------------------------------------------------------------------
# the GPU cases

@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("M, D, fmt, n_taps, taps, S", CHAN_CASES)
def test_chan_instantiation(api, L, M, D, fmt, n_taps, taps, S):
    rng = np.random.default_rng([M, D, n_taps, S])
    h = _taps(taps, n_taps, 1.0 / M, rng)
    n_out = chan_length(M, D, n_taps)
    assert _covered(chan_layout(M, D, n_taps, n_out)[1])
    n = n_out * D
    in_stride, out_stride = n + 38, n_out + 3
    lib = L.load()
    if fmt == "cf32":
        x = np.stack([synth.synth_cf32(n, ch=s).view(np.complex64) for s in range(S)])
        d_in = _padded(api, x, in_stride, np.nan)
        at, isz = d_in.ptr, 8
    else:
        b = rng.integers(0, 256, size=(S, 2 * in_stride), dtype=np.uint8)
        d_in, at = _u8_input(api, lib, b, 2 if M.bit_length() % 2 else 6)
        isz = 2
        x = _u8_decode(b[:, :2 * n])
    hist = api.chan_plan(n_taps, M, D)[1] // D

    def run(cuts, u8=fmt == "u8", at=at, isz=isz):
        ch = api.Chan(h, M, D, n_streams=S)
        if u8:
            ch.set_input_format(L.FMT_U8)
        d_out, o = _filled(api, 2 * S * M * out_stride, SENT)
        pos = 0
        for c in cuts:
            assert ch.process_stream(at + isz * D * pos, c * D, o + 8 * pos, in_stride=in_stride, out_stride=out_stride) == c
            pos += c
        y = _rows(d_out, SENT, S * M, 2 * out_stride, 2 * n_out)
        ch.close()
        d_out.free()
        return y

    one = run([n_out])
    y = _cf32(one).reshape(S, M, n_out)
    for s in range(S):
        _check(y[s], _chan_reference(x[s], h, M, D), (M, D, fmt, n_taps, s))
    if fmt == "u8":
        # the same bytes through the library's converter and the cf32 instantiation give the same bits
        d_b = api.DeviceArray.from_bytes(b)
        d_f = api.DeviceArray(b.size)
        assert lib.sfe_dsp_rx_u8_to_f32(d_b.ptr, d_f.ptr, b.size, None) == 0
        assert np.array_equal(run([n_out], u8=False, at=d_f.ptr, isz=8), one)
        d_b.free()
        d_f.free()
    cuts = _cuts(n_out, hist)
    assert np.array_equal(run(cuts), one), cuts
    d_in.free()


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("M, D, n_taps, taps, S", COMBINE_CASES)
def test_combine_instantiation(api, L, M, D, n_taps, taps, S):
    rng = np.random.default_rng([M, D, n_taps, S])
    g = _taps(taps, n_taps, 1.0 / M, rng)
    hist = api.combine_plan(n_taps, M, D)[1]
    logj = (hist + 1).bit_length() - 1
    n = combine_length(M, D, logj)
    G, _, kinds = combine_layout(M, D, logj, n)
    assert _covered(kinds) and n * S <= 32 * G << logj
    n_out = n * D
    in_stride = n + 5
    # channel k of stream s is synth stream s M + k (uniform, variance 1/3 per part), scaled for an output RMS of about
    # 0.35 per part: the TX10 codes swing across their range
    scale = 0.35 / np.sqrt(M * np.sum(g.astype(np.float64) ** 2) / D / 3.0)
    X = np.stack([np.stack([synth.synth_cf32(n, ch=s * M + k).view(np.complex64) for k in range(M)]) for s in range(S)])
    X = (X * np.float32(scale)).astype(np.complex64)
    d_in = _padded(api, X.reshape(S * M, n), in_stride, np.nan)
    lib = L.load()

    def run(cuts, tx10):
        cb = api.Combiner(g, M, D, n_streams=S)
        if tx10:
            cb.set_output_format(L.FMT_TX10)
        out_stride = n_out + (6 if tx10 else 5)            # TX10 takes whole 5-byte groups per stream: an even stride
        row_b, used_b, word = (out_stride // 2 * 5, n_out // 2 * 5, SENT_TX10) if tx10 else (8 * out_stride, 8 * n_out, SENT)
        d_out, o = _filled(api, _ceil(S * row_b, 4), word)
        pos = 0
        for c in cuts:
            po = o + (pos * D // 2 * 5 if tx10 else 8 * pos * D)
            assert cb.process_stream(d_in.ptr + 8 * pos, c, po, in_stride=in_stride, out_stride=out_stride) == c * D
            pos += c
        y = _rows(d_out, word, S, row_b, used_b, np.uint8) if tx10 else _rows(d_out, word, S, row_b // 4, used_b // 4)
        cb.close()
        d_out.free()
        return y

    one = run([n], False)
    z = _cf32(one)
    for s in range(S):
        ref = _combine_reference(X[s], g, M, D)
        _check(z[s].reshape(n, D).T, ref.reshape(n, D).T, (M, D, n_taps, s))   # rows: the D output phases
    cuts = _cuts(n, hist)
    assert np.array_equal(run(cuts, False), one), cuts
    # TX10: the bytes sfe_dsp_tx_f32_to_10bit makes of the F32 output, in one call and in the cut list
    d_f = api.DeviceArray.from_numpy(one.view(np.float32))
    d_b = api.DeviceArray(_ceil(S * n_out // 2 * 5, 4) + 1)
    assert lib.sfe_dsp_tx_f32_to_10bit(d_f.ptr, d_b.ptr, 2 * S * n_out, None) == 0
    want = d_b.to_numpy().view(np.uint8)[:S * n_out // 2 * 5].reshape(S, n_out // 2 * 5)
    d_f.free()
    d_b.free()
    assert np.array_equal(run([n], True), want)
    assert np.array_equal(run(cuts, True), want), cuts
    d_in.free()


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt, D, K, n_taps, taps, S", DDC_CASES)
def test_ddc_instantiation(api, L, fmt, D, K, n_taps, taps, S):
    rng = np.random.default_rng([D, K, n_taps, S])
    h = _taps(taps, n_taps, 0.5 / D, rng)
    f = rng.uniform(-0.5, 0.5, K)
    if K >= 3:
        f[:3] = (0.5, -0.5, 0.0)
    incs = synth.ddc_incs(f)
    n_out = ddc_length(D, K, n_taps)
    assert _covered(ddc_layout(D, K, n_taps, n_out)[1])
    n = n_out * D
    in_stride, out_stride = n + 38, n_out + 3
    lib = L.load()
    if fmt == "cf32":
        x = np.stack([synth.synth_cf32(n, ch=s).view(np.complex64) for s in range(S)])
        d_in = _padded(api, x, in_stride, np.nan)
        at, isz = d_in.ptr, 8
    elif fmt == "real":
        x = np.stack([synth.synth_f32(n, ch=s) for s in range(S)])
        d_in = _padded(api, x, in_stride, np.nan)
        at, isz = d_in.ptr, 4
    else:
        b = rng.integers(0, 256, size=(S, 2 * in_stride), dtype=np.uint8)
        d_in, at = _u8_input(api, lib, b, 2 if D % 2 else 6)
        isz = 2
        x = _u8_decode(b[:, :2 * n])
    hist = api.ddc_plan(n_taps, D, f)[1] // D

    def run(cuts):
        dd = api.Ddc(h, D, f, data_complex=fmt != "real", n_streams=S)
        if fmt == "u8":
            dd.set_input_format(L.FMT_U8)
        d_out, o = _filled(api, 2 * S * K * out_stride, SENT)
        pos = 0
        for c in cuts:
            assert dd.process_stream(at + isz * D * pos, c * D, o + 8 * pos, in_stride=in_stride, out_stride=out_stride) == c
            pos += c
        y = _rows(d_out, SENT, S * K, 2 * out_stride, 2 * n_out)
        dd.close()
        d_out.free()
        return y

    one = run([n_out])
    y = _cf32(one).reshape(S, K, n_out)
    for s in range(S):
        _check(y[s], synth.ddc_reference(x[s], h, D, incs), (fmt, D, K, n_taps, s))
    cuts = _cuts(n_out, hist)
    assert np.array_equal(run(cuts), one), cuts
    d_in.free()


# ------------------------------------------------------------------------------------------------------------------------
# without a GPU: the tables against the compiled instantiations, and the restated tile rules against the sources

def _instantiations(name):
    """Template arguments of every `name<...>` kernel that build/<file>.resources.json lists."""
    from simplefe_amd import build
    build.build_lib()
    res = json.load(open(os.path.join(build.HERE, "build", name.split("_")[0] + ".hip.resources.json")))
    return {tuple(a.strip() for a in re.search(name + r"<(.*?)>", k).group(1).split(",")) for k in res if name + "<" in k}


def _b(v):
    return "true" if v else "false"


def test_tables_cover_every_instantiation():
    """Every case maps to the instantiation the host selects for it, every call reaches its edge and interior tiles,
    and the union of the cases is the set of instantiations compiled: a case dropped from a table, or an instantiation
    added without a case, fails here."""
    from simplefe_amd import api
    chan = set()
    for M, D, fmt, n_taps, _, _ in CHAN_CASES:
        assert _covered(chan_layout(M, D, n_taps, chan_length(M, D, n_taps))[1]), (M, D, n_taps)
        chan.add((str(M.bit_length() - 1), _b(D != M), _b(fmt == "u8")))
    assert len(chan) == len(CHAN_CASES) and chan == _instantiations("chan_kernel")
    for M in {c[0] for c in CHAN_CASES}:
        taps = [c[3] for c in CHAN_CASES if c[0] == M]
        assert {_ceil(_ceil(t, M), 8) * 8 for t in taps} == {8, 16, 24, 32} and 32 * M in taps, M
        assert any(t % M == 1 for t in taps), M

    combine, P = set(), set()
    for M, D, n_taps, _, S in COMBINE_CASES:
        hist = api.combine_plan(n_taps, M, D)[1]
        logj = (hist + 1).bit_length() - 1
        assert hist == (1 << logj) - 1, (M, D, n_taps, hist)
        n = combine_length(M, D, logj)
        G, _, kinds = combine_layout(M, D, logj, n)
        assert _covered(kinds) and n * S <= 32 * G << logj, (M, D, n_taps, kinds)
        combine.add((str(M.bit_length() - 1), _b(D != M), str(logj)))
        P.add((D != M, _ceil(n_taps, D)))
    assert len(combine) == len(COMBINE_CASES) and combine == _instantiations("combine_kernel")
    assert {(False, 9), (False, 17), (True, 9), (True, 17), (True, 33), (False, 32), (True, 64)} <= P
    assert {(1024, 1024, 32768), (1024, 512, 32768)} <= {c[:3] for c in COMBINE_CASES}

    ddc = set()
    for fmt, D, K, n_taps, _, _ in DDC_CASES:
        assert _covered(ddc_layout(D, K, n_taps, ddc_length(D, K, n_taps))[1]), (fmt, D, K, n_taps)
        kt = ddc_tunings_per_chunk(K)
        ddc |= {(str(DDC_FORMATS[fmt]), str(kt), str(16 if kt <= 2 else 8), _b(g)) for g in (False, True)}
    assert ddc == _instantiations("ddc_kernel")
    assert {c[2] for c in DDC_CASES} == {1, 2, 3, 4, 5, 8, 9, 63, 64}
    assert {c[1] for c in DDC_CASES} == {1, 2, 7, 255, 256, 257, 1023, 1024}
    P = [_ceil(c[3], c[1]) for c in DDC_CASES]
    assert max(P) == 64 and sum(p % 4 == 1 for p in P) >= 3


# the source lines that chan_layout, combine_layout, ddc_layout and ddc_tunings_per_chunk restate (whitespace aside): a
# change to a tile rule fails here until the restatement, and with it the call lengths, follows it
TILE_RULES = {
    "chan.hip": [
        "int chan_tile_rows(int logm) { return logm <= 8 ? 16 * (256 >> logm) : 8; }",
        "const bool interior = (mtile - (long long)SH * (a.P - 1)) * D - (M - 1) >= 0 && mtile + ROWS <= a.n_out;",
    ],
    "api_chan.hip": [
        "constexpr int CHAN_RU = 8;",
        "c->Ppad = (c->P + CHAN_RU - 1) / CHAN_RU * CHAN_RU;",
    ],
    "combine.hip": [
        "constexpr int comb_cs(int logm, bool half, int logj) { return logm == 10 && logj == (half ? 6 : 5) ? 2 : 1; }",
        "constexpr int comb_cols(int logm, bool half, int logj) { return (half ? (1 << logm) / 2 : 1 << logm) / "
        "comb_cs(logm, half, logj); }",
        "constexpr int comb_threads(int logm, bool half, int logj) { return comb_cols(logm, half, logj) > 256 ? "
        "comb_cols(logm, half, logj) : 256; }",
        "constexpr int comb_rows(int logm, int logj) { return (logm <= 8 ? 4096 >> logm : 8) >> (logj == 6 ? 1 : 0); }",
        "constexpr int NT = comb_threads(LOGM, HALF, LOGJ), G = NT / DC;",
        "constexpr int ROWS = comb_rows(LOGM, LOGJ), RG = ROWS / G, RS = M + 1;",
        "constexpr int W0 = (J - 1 + RG - 1) / RG * RG;",
        "if (m00 >= 0 && m00 + (G - 1) * run + RG <= n_in) {",
        "const int n_chunks = (W0 + run) / RG;",
    ],
    "api_combine.hip": [
        "const long long want_wg = 8LL * device_cu_count();",
        "long long run = ((long long)n_in * c->n_streams + want_wg * segs - 1) / (want_wg * segs);",
        "run = std::max(run, 4LL * (1 << c->logj)); run = std::min(run, (long long)n_in); run = (run + rg - 1) / rg * rg;",
    ],
    "ddc.hip": [
        "enum { DDC_CF32 = 0, DDC_U8 = 1, DDC_REAL = 2 };",
        "constexpr int ddc_instants(int kt) { return kt >= 4 ? 8 : 16; }",
        "int ddc_tunings_per_chunk(int K) { return K == 1 ? 1 : K == 2 ? 2 : K <= 4 ? 4 : 8; }",
        "const int rows = (DDC_THREADS / (D < DDC_THREADS ? D : DDC_THREADS)) * ddc_instants(kt);",
        "const int m_lo = P - 1 + (D > 1), t_lo = (int)std::min<long long>(tiles, (m_lo + rows - 1) / rows);",
        "const int t_hi = std::max(t_lo, n_out / rows);",
    ],
    "api_ddc.hip": [
        "constexpr int DDC_RU = 4;",
        "c->Ppad = (c->P + DDC_RU - 1) / DDC_RU * DDC_RU;",
        "const int fmt = c->in_u8 ? 1 : c->complex_in ? 0 : 2;",
    ],
}


def test_tile_rules_follow_the_sources():
    for name, lines in TILE_RULES.items():
        text = re.sub(r"\s+", " ", open(os.path.join(CSRC, name)).read())
        for line in lines:
            assert re.sub(r"\s+", " ", line) in text, (name, line)
