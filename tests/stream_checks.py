"""Poisoned, guarded buffers and strict verdicts for the FIR / resampler / decimator stream calls.

Two layers:

  * verdict functions in plain numpy (no GPU, nothing from oracle/): check_written, check_input_intact,
    check_counts, check_values, and the two per-sample bounds direct_bound / transform_bound;
  * GPU runners run_rs / run_fir, which make the calls Rs.resample_array / Fir.filter make, but into an output that
    is poisoned before EVERY call and sits between guards, from an input that sits at an offset inside a larger
    buffer whose every other word is NaN; after each call both buffers are read back whole and judged;
  * run_psd / run_corr / run_iir, the same for the three streaming measurement blocks, with a gap between the streams of
    the input and between the rows of every output as well (tests/test_measure_checks_host.py holds their negative controls).

Each verdict raises its own exception (all of them AssertionErrors), so a negative control can tell WHICH check
caught a corruption: WrittenError, InputError, CountError, ValuesError (its .gate names the gate that failed:
"shape", "exact", "rms" or "sample").

The poison is a quiet NaN with a payload (0x7fd5a5a5).  No finite arithmetic produces it, so "still poison" means
"never stored" and "no longer poison" means "stored", bit for bit.

The per-sample gate
-------------------
rel-RMS over a long stream cannot see one wrong sample (one of 250 001 off by 0.1 % moves it by 8e-7); a dropped
end tap or a wrong halo sample at a tile edge is exactly that.  So beside the rel-RMS gate every output is held
to a bound of its own, derived from the arithmetic and not from what the kernels were seen to do.

Direct sums (polyphase.hip, poly_rt_dma.hip, the FIR's direct kernel, poly_seg_kernel), against a float32
reference that adds the same L products:

    |got - ref| <= 2 (L + 3) 2^-24 A + 1e-30        A = the same operation on |taps| and |x|

A float32 sum of L products, in any order, fused or not, is within (L + 1) u A of the exact value to first order
(u = 2^-24: one rounding per product, at most L - 1 per partial sum, worst case every one of them on the critical
path); the blend out = s0 (1 - mu) + mu s1 adds three roundings; got and ref each carry that error, hence the 2.
Against a float64 reference the same bound has a factor of two to spare.  DECIMATE mode folds nothing: the class
keeps the caller's taps as they are (libdsp/decimate.cxx:37-59 copies them and pads an even count with one zero
tap; get_sample, :132-139, sums taps[phase + j U] x[n - j]), every weight is one tap, so the operation on |taps|
and |x| dominates there as in RESAMPLE mode.

Transform-domain kernels (fir_fft.hip, poly_gen.hip: one 4096-point complex transform per block; poly_fft.hip:
256-point transforms of the stream's SP polyphase components), against any reference that is itself far more
accurate than the bound:

    |got - ref| <= log2(N) 2^-24 ||x_window||_2 (17 ||h||_2 + 8 ||h||_1) + 1e-30

y = IDFT(DFT(x) H).  A float32 Cooley-Tukey transform of length N errs by at most log2(N) eta ||.||_2 normwise,
eta = mu + gamma_4 (sqrt 2 + mu) (Higham, Accuracy and Stability of Numerical Algorithms, thm 24.2); with
twiddles good to a few u that is about 6.4 u, taken as 8 u.  Four terms reach an output sample n, with
|IDFT(D H)[n]| <= ||D||_2 ||H||_2 / N and ||X||_2 = sqrt N ||x||_2:
    forward transform   dX,  ||dX|| <= 8 log2 N u ||X||      ->  8 log2 N u ||x|| ||h||_2
    the taps' spectrum  dH,  the same                        ->  8 log2 N u ||x|| ||h||_2
    the bin products, sqrt 5 u each                          ->  2.3 u ||x|| ||h||_2     (< 1 log2 N u for N >= 8)
    inverse transform   <= 8 log2 N u ||y_circular||_2,  and ||y_circular||_2 <= ||h||_1 ||x||_2 (Young)
which add up to the line above: c = 17 on ||h||_2 and 8 on ||h||_1.  x_window is what one transform holds; which
block an output falls in is the kernel's business, so the window used here is every sample within one transform
length on either side of the output (a superset of any block that holds it: at most sqrt 2 more than needed).
For the resamplers h is the polyphase branch (the worst branch's norms; an output blends two branches with
weights that add up to 1, the blend's three roundings fit in the term to spare); for poly_fft.hip the SP
component convolutions add up to the same form by Cauchy-Schwarz over the components, with N = 256 and a window
of 256 SP input samples; a real stream through poly_gen.hip rides two blocks per transform (window 2 N).
tests/test_stream_checks_host.py checks that float32 overlap-save by scipy.fft at the same lengths stays inside.
What this gate can and cannot see: it is a worst-case bound, the ||h||_1 term and the two-sided window included, and a
float32 transform's real error sits some three orders of magnitude under it (the host test prints 1e-4 to 2e-3 of the
bound); it allows about 5e-4 of the block's scale per sample.  So on the transform-domain kernels it catches a sample
that is grossly wrong -- a dropped block edge, a stale or unscaled value -- and NOT one that is off by 0.1 %; those
kernels' fine errors are left to the rel-RMS gate and to the exact-mode twins that share their launch geometry.  Where a
test cannot know which kernel served a call (K >= 4096 at an integer step, a general rate at a small blksize) and takes
the wider of the two bounds, a direct kernel serving that call is held only to the loose one.
"""
import numpy as np

POISON = 0x7FD5A5A5
U24 = 2.0 ** -24
RMS_TOL = 1e-5


class WrittenError(AssertionError):
    pass


class InputError(AssertionError):
    pass


class CountError(AssertionError):
    pass


class ValuesError(AssertionError):
    def __init__(self, gate, msg):
        super().__init__("%s gate: %s" % (gate, msg))
        self.gate = gate


# ------------------------------------------------------------------------------------------------ layouts
class Layout:
    """Where the channels of one buffer sit, in BYTES: channel c owns [front + c*stride, front + c*stride + cap),
    items of `item` bytes, judged in cells of `gran` bytes (a float32 word; a 5-byte group of the TX10 format).
    Everything else -- the front guard, the gaps between channels, the tail guard -- belongs to nobody."""

    def __init__(self, n_channels, item, cap_items, stride_items, front, tail, gran=4):
        assert stride_items >= cap_items
        self.n_channels, self.item, self.gran = int(n_channels), int(item), int(gran)
        self.cap_items, self.stride_items = int(cap_items), int(stride_items)
        self.front, self.stride, self.cap = int(front), int(stride_items) * int(item), int(cap_items) * int(item)
        used = self.front + (self.n_channels - 1) * self.stride + self.cap + int(tail)
        self.words = (used + 3) // 4
        self.total = 4 * self.words

    def start(self, c):
        return self.front + c * self.stride

    def poisoned(self):
        return np.full(self.words, POISON, dtype=np.uint32)

    def put(self, raw, c, data, at_item=0):
        """Lay `data` (any dtype, raw bytes) into channel c from item `at_item` on; raw is the uint32 buffer."""
        b = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        o = self.start(c) + at_item * self.item
        raw.view(np.uint8)[o:o + b.size] = b

    def take(self, raw, c, k, dtype=np.float32):
        o = self.start(c)
        return raw.view(np.uint8)[o:o + k * self.item].copy().view(dtype)


def out_layout(n_channels, item, cap_items, gran=4, guard=256, gap_items=5, quantum=16):
    """A front guard, out_stride > out_cap and a tail guard; channels start on 16-byte boundaries."""
    stride = -(-(cap_items + gap_items) // quantum) * quantum
    return Layout(n_channels, item, cap_items, stride, guard, guard, gran)


def in_layout(n_channels, item, n_items, aligned=True, lead=64, gap_items=7, quantum=16):
    """The samples at an offset inside a larger buffer.  aligned: every channel starts on a 16-byte boundary (the
    kernels that fetch tiles by 16-byte DMA lanes); else one sample on, at an odd stride (the kernels they replace)."""
    stride = -(-(n_items + gap_items) // quantum) * quantum
    front = lead
    if not aligned:
        stride += 1
        front += item
    return Layout(n_channels, item, n_items, stride, front, 64, 4)


# ------------------------------------------------------------------------------------------------ verdicts
def _same_as_poison(raw):
    raw = np.ascontiguousarray(raw)
    assert raw.dtype == np.uint32
    return raw.view(np.uint8) == np.full(raw.size, POISON, dtype=np.uint32).view(np.uint8)


def check_written(raw, layout, k):
    """raw: the whole read-back output buffer as uint32; k items per channel were reported written.  Every cell of
    each channel's [0, k) differs from the poison; every byte outside the channels' declared ranges [0, cap) still is
    the poison; [k, cap) is free (include/sfe_dsp.h: up to out_cap outputs per channel may be written)."""
    same = _same_as_poison(raw)
    if same.size != layout.total:
        raise WrittenError("buffer of %d bytes, layout of %d" % (same.size, layout.total))
    if k * layout.item > layout.cap:
        raise WrittenError("%d items reported, the declared range holds %d" % (k, layout.cap_items))
    owned = np.zeros(same.size, dtype=bool)
    for c in range(layout.n_channels):
        o = layout.start(c)
        owned[o:o + layout.cap] = True
        nb = k * layout.item
        cells = same[o:o + nb - nb % layout.gran].reshape(-1, layout.gran).all(axis=1)
        if cells.any():
            i = int(np.flatnonzero(cells)[0])
            raise WrittenError("channel %d: cell %d of %d (item %d of %d) was never stored (%d cells in all)"
                               % (c, i, cells.size, i * layout.gran // layout.item, k, int(cells.sum())))
    stray = ~same & ~owned
    if stray.any():
        o = int(np.flatnonzero(stray)[0])
        if o < layout.front:
            where = "the front guard, %d bytes before channel 0" % (layout.front - o)
        elif o >= layout.start(layout.n_channels - 1) + layout.cap:
            where = "the tail guard, %d bytes past the declared range" % (o - layout.start(layout.n_channels - 1) - layout.cap)
        else:
            c = (o - layout.front) // layout.stride
            where = "the gap after channel %d, %d bytes past its out_cap" % (c, o - layout.start(c) - layout.cap)
        raise WrittenError("a store outside the declared range: byte %d, in %s (%d bytes in all)" % (o, where, int(stray.sum())))


def check_input_intact(raw_in_after, raw_in_before):
    """Bit equality of the whole input buffer, surroundings included."""
    a, b = np.ascontiguousarray(raw_in_after).view(np.uint8), np.ascontiguousarray(raw_in_before).view(np.uint8)
    if a.size != b.size:
        raise InputError("input buffer changed size: %d -> %d bytes" % (b.size, a.size))
    d = a != b
    if d.any():
        raise InputError("the input buffer changed: %d bytes, the first at byte %d" % (int(d.sum()), int(np.flatnonzero(d)[0])))


def closed_form_total(n, U, S):
    """Outputs of n samples from a fresh start at an integer-valued step S on the grid upsampled by U: output j sits
    at j S and is emitted while j S <= n U - 2 (libdsp/resample.cxx:137-146)."""
    return max(0, (n * U - 2) // S + 1) if n * U >= 2 else 0


def check_counts(per_call, ref, state, n, U, S):
    """per_call: the counts the calls reported.  ref: the reference's total, or its per-call list when it was fed the
    same calls.  state: the handle's time state after the last call (anything with .leftover), or None.  n samples per
    channel in all; S: the integer-valued step rate*U, or None for a general rate.  No slack anywhere."""
    per_call = [int(v) for v in per_call]
    total = sum(per_call)
    if np.ndim(ref) == 0:
        ref_total = int(ref)
    else:
        ref = [int(v) for v in ref]
        ref_total = sum(ref)
        if len(ref) == len(per_call) and ref != per_call:
            raise CountError("per call %s, the reference %s" % (per_call, ref))
    if total != ref_total:
        raise CountError("%d outputs in all, the reference has %d" % (total, ref_total))
    if S is not None:
        K = closed_form_total(n, U, S)
        if total != K:
            raise CountError("%d outputs in all, the closed form (n U - 2) // S + 1 gives %d (n %d, U %d, S %d)" % (total, K, n, U, S))
        if state is not None and bool(state.leftover) != (K * S - n * U == -1):
            raise CountError("leftover %d after the last call; K S - n U = %d" % (int(state.leftover), K * S - n * U))


def int_step(rate, U):
    """The integer-valued step fl(rate * U) of the float32 law, or None for a general rate."""
    step = float(np.float32(rate) * np.float32(U))
    return int(step) if step >= 1.0 and step == np.floor(step) else None


def check_total(k, ref_total, n, U, rate, state=None):
    """check_counts for one stream's total: k outputs of n samples against the reference's count."""
    check_counts([k], ref_total, state, n, U, int_step(rate, U))


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.sum((a - b) ** 2) / max(np.sum(b ** 2), 1e-300)))


def check_values(got, ref, exact=False, bound=None, tol=RMS_TOL, label=""):
    """exact: uint32 equality (the sign of a zero included).  Else the rel-RMS gate (tol) AND, with `bound` (one value
    per output, or a scalar), the per-sample gate |got - ref| <= bound.  Returns the worst |got - ref| / bound."""
    got, ref = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(ref, dtype=np.float32)
    if got.shape != ref.shape:
        raise ValuesError("shape", "%s got %s, reference %s" % (label, got.shape, ref.shape))
    if exact:
        d = got.view(np.uint32) != ref.view(np.uint32)
        if d.any():
            i = int(np.flatnonzero(d.ravel())[0])
            raise ValuesError("exact", "%s %d of %d words differ, the first at %d: %r != %r" % (label, int(d.sum()), d.size, i, got.ravel()[i], ref.ravel()[i]))
        return 0.0
    if not (np.isfinite(got).all()):
        i = int(np.flatnonzero(~np.isfinite(got.ravel()))[0])
        raise ValuesError("rms", "%s a NaN or infinity at %d (%d in all)" % (label, i, int((~np.isfinite(got)).sum())))
    e = rel_rms(got, ref)
    if not e <= tol:
        raise ValuesError("rms", "%s rel-RMS %.3g > %.3g" % (label, e, tol))
    if bound is None:
        return 0.0
    b = np.broadcast_to(np.asarray(bound, np.float64), got.shape)
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    ratio = d / b
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        i = int(np.argmax(ratio.ravel()))
        raise ValuesError("sample", "%s output %d: |%r - %r| = %.3g is %.3g x its bound (%d of %d outside)"
                          % (label, i, got.ravel()[i], ref.ravel()[i], d.ravel()[i], worst, int((ratio > 1).sum()), d.size))
    return worst


def direct_bound(A, L):
    """2 (L + 3) 2^-24 A + 1e-30: A the same operation on |taps| and |x|, L taps per output sum."""
    return 2.0 * (L + 3) * U24 * np.abs(np.asarray(A, np.float64)) + 1e-30


def phase_norms(taps, U=1):
    """(worst branch ||h||_2, worst branch ||h||_1) of the U polyphase branches taps[j::U]."""
    t = np.asarray(taps)
    return (max(float(np.sqrt(np.sum(np.abs(t[j::U].astype(np.complex128)) ** 2))) for j in range(U)),
            max(float(np.sum(np.abs(t[j::U].astype(np.complex128)))) for j in range(U)))


def transform_bound(x, taps, N, window, positions, U=1, cplx=False):
    """log2(N) 2^-24 ||x_window||_2 (17 ||h||_2 + 8 ||h||_1) + 1e-30 per output: x one channel's samples (interleaved
    I/Q with cplx), positions[k] the input sample output k is taken at, `window` samples on either side of it."""
    x = np.asarray(x, np.float64)
    p2 = x[0::2] ** 2 + x[1::2] ** 2 if cplx else x ** 2
    cs = np.concatenate([[0.0], np.cumsum(p2)])
    p = np.asarray(positions, np.int64)
    lo, hi = np.clip(p - window, 0, p2.size), np.clip(p + window + 1, 0, p2.size)
    xw = np.sqrt(np.maximum(cs[hi] - cs[lo], 0.0))
    h2, h1 = phase_norms(taps, U)
    b = np.log2(N) * U24 * xw * (17.0 * h2 + 8.0 * h1) + 1e-30
    return np.repeat(b, 2) if cplx else b


def reference_calls(cuts, B):
    """The reference calls behind the bulk calls [cuts[i], cuts[i+1]): each is replayed in blksize-sample calls from
    its own start (include/sfe_dsp.h, sfe_dsp_rs_process_stream).  Returns a list of lists of (a, b)."""
    return [[(a, min(a + B, e)) for a in range(s, e, B)] for s, e in zip(cuts[:-1], cuts[1:])]


def reference_stream(obj, x, rate, cuts, B):
    """Feed a reference object (anything with process(x, out_len, rate) -> (n, out)) the calls the bulk calls replay;
    returns (outputs, the count of each bulk call)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    ys, ns = [np.zeros(0, np.float32)], []
    for calls in reference_calls(cuts, B):
        k = 0
        for a, b in calls:
            n, o = obj.process(x[a:b], int(np.ceil((b - a) / rate)) + 2, rate)
            ys.append(o[:n])
            k += n
        ns.append(k)
    return np.concatenate(ys), ns


def law_positions(n, U, rate, cuts, B):
    """The reference's float32 time law (libdsp/resample.cxx:89,119-150) replayed in numpy float32 over the reference
    calls behind the bulk calls `cuts`: (positions on the upsampled grid from the stream's start, mu, the count of each
    bulk call, leftover after the last call).  A leftover output sits one grid point before its call."""
    f32 = np.float32
    step = f32(rate) * f32(U)
    pos, mu, left = 0, f32(0.0), False
    P, M, counts = [], [], []
    for calls in reference_calls(cuts, B):
        k0 = len(P)
        for a, b in calls:
            m = b - a
            t = f32(pos) + mu
            if left:
                P.append(a * U - 1)
                M.append(mu)
                left = False
                t = f32(t + step)
            while True:
                pos = int(np.floor(t))
                mu = f32(t - f32(pos))
                n0, n1 = int(pos / U), int((pos + 1) / U)          # C truncation
                if n0 >= m:
                    break
                if n1 >= m:
                    left = True
                    break
                P.append(a * U + pos)
                M.append(mu)
                t = f32(t + step)
            pos -= m * U
        counts.append(len(P) - k0)
    return np.array(P, np.int64), np.array(M, np.float64), counts, left


def direct_resample64(x, taps, U, pos, mu):
    """out = s(p) (1 - mu) + mu s(p + 1), s(p) = sum_j taps[p % U + j U] x[p // U - j], in float64, zeros before the
    stream: the plain high-precision statement of the law at the given (position, mu) sequence."""
    x, taps = np.asarray(x, np.float64), np.asarray(taps, np.float64)
    L = -(-taps.size // U)
    T = np.zeros((U, L))
    for j in range(U):
        T[j, : taps[j::U].size] = taps[j::U]
    xp = np.concatenate([np.zeros(L + 1), x, np.zeros(2)])

    def s(p):
        out = np.empty(p.size)
        for i in range(0, p.size, 8192):
            q = p[i:i + 8192]
            idx = (q // U + L + 1)[:, None] - np.arange(L)[None, :]
            out[i:i + 8192] = np.einsum("kl,kl->k", T[q % U], xp[idx])
        return out

    pos, mu = np.asarray(pos, np.int64), np.asarray(mu, np.float64)
    return s(pos) * (1.0 - mu) + mu * s(pos + 1)


# ------------------------------------------------------------------------------------------------ GPU runners
def _upload(api, raw):
    return api.DeviceArray.from_numpy(np.ascontiguousarray(raw).view(np.float32))


def _download(d):
    return d.to_numpy().view(np.uint32)


def _cuts(cuts, n):
    if cuts is None:
        return [0, n]
    if np.ndim(cuts) == 0:
        return sorted(set(list(range(0, n, int(cuts))) + [n])) if n else [0, 0]
    return [int(v) for v in cuts]


def _lay_input(x, nch, item, a, b, aligned):
    lay = in_layout(nch, item, b - a, aligned=aligned)
    raw = lay.poisoned()
    rows = np.ascontiguousarray(x).reshape(nch, -1).view(np.uint8)
    for c in range(nch):
        lay.put(raw, c, rows[c, a * item:b * item])
    return lay, raw


def run_rs(api, r, x, rate, cuts=None, in_u8=False, aligned=True, cap=None):
    """Rs.resample_array through poisoned, guarded buffers: x (n_channels, n*) float32 (interleaved I/Q when complex;
    uint8 with in_u8), fed in the calls [cuts[i], cuts[i+1]) (None: one call; an int: calls of that many samples).
    Returns ((n_channels, n_out*) float32, the per-call counts).  At an integer-valued step every call's count and the
    state it leaves are also held to the law replayed here from the state the handle was found in: output j of a call
    sits at p0 + j S (p0 = -1 for a pending leftover) and is emitted while <= m U - 2."""
    nch, w = r.n_channels, 2 if r.data_complex else 1
    x = np.ascontiguousarray(x, dtype=np.uint8 if in_u8 else np.float32).reshape(nch, -1)
    item = w * (1 if in_u8 else 4)
    n = x.shape[1] // w
    cuts = _cuts(cuts, n)
    S = int_step(rate, r.upsample)
    p0 = None
    if S is not None:
        st = r.get_state()
        if st.mu == 0.0:
            p0 = -1 if st.leftover else int(st.pos)
    outs, counts = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        m = b - a
        ilay, iraw = _lay_input(x, nch, item, a, b, aligned)
        # room: m / rate outputs, and what the float32 recurrence's drift can add per reference call at a general rate
        kcap = int(cap) if cap is not None else int(np.ceil(m / rate)) + 4 + (0 if S is not None else 2 * (m // r.blksize + 1))
        olay = out_layout(nch, 4 * w, kcap)
        d_in, d_out = _upload(api, iraw), _upload(api, olay.poisoned())
        try:
            k = r.process_stream(d_in.ptr + ilay.front, m, d_out.ptr + olay.front, kcap, rate,
                                 in_stride=ilay.stride_items, out_stride=olay.stride_items)
            oraw, iafter = _download(d_out), _download(d_in)
        finally:
            d_in.free()
            d_out.free()
        check_written(oraw, olay, k)
        check_input_intact(iafter, iraw)
        if p0 is not None:
            lim = m * r.upsample - 2
            want = (lim - p0) // S + 1 if p0 <= lim else 0
            p0 += want * S - m * r.upsample
            st = r.get_state()
            if k != want or bool(st.leftover) != (p0 == -1) or (p0 != -1 and st.pos != p0):
                raise CountError("call [%d, %d): %d outputs, state (pos %d, leftover %d); the law gives %d and position %d"
                                 % (a, b, k, st.pos, st.leftover, want, p0))
        counts.append(k)
        outs.append(np.stack([olay.take(oraw, c, k) for c in range(nch)]))
    y = np.concatenate(outs, axis=1) if outs else np.zeros((nch, 0), np.float32)
    return y, counts


def run_fir(api, f, x, cuts=None, in_u8=False, out_tx10=False, aligned=True):
    """Fir.filter through poisoned, guarded buffers: x (n_channels, n*) float32 (uint8 with in_u8), fed in the calls
    [cuts[i], cuts[i+1]).  Returns (n_channels, n*) float32, or with out_tx10 the (n_channels, bytes) uint8 groups (the
    cuts then fall on whole groups).  The declared output range of a channel is the call's n samples."""
    nch, w, wo = f.n_channels, 2 if f.data_complex else 1, 2 if f.out_complex else 1
    x = np.ascontiguousarray(x, dtype=np.uint8 if in_u8 else np.float32).reshape(nch, -1)
    item = w * (1 if in_u8 else 4)
    n = x.shape[1] // w
    cuts = _cuts(cuts, n)
    per_group = 4 // wo                                   # samples in a 5-byte TX10 group
    outs = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        m = b - a
        ilay, iraw = _lay_input(x, nch, item, a, b, aligned)
        if out_tx10:
            assert a % per_group == 0
            groups = m // per_group
            olay = out_layout(nch, 5, groups, gran=5, quantum=16)
            out_stride, k = olay.stride_items * per_group, groups
        else:
            olay = out_layout(nch, 4 * wo, m)
            out_stride, k = olay.stride_items, m
        d_in, d_out = _upload(api, iraw), _upload(api, olay.poisoned())
        try:
            f.process_stream(d_in.ptr + ilay.front, d_out.ptr + olay.front, m, in_stride=ilay.stride_items, out_stride=out_stride)
            oraw, iafter = _download(d_out), _download(d_in)
        finally:
            d_in.free()
            d_out.free()
        check_written(oraw, olay, k)
        check_input_intact(iafter, iraw)
        outs.append(np.stack([olay.take(oraw, c, k, np.uint8 if out_tx10 else np.float32) for c in range(nch)]))
    return np.concatenate(outs, axis=1) if outs else np.zeros((nch, 0), np.float32)


def resample_array(api, r, x, rate, chunk=None, **kw):
    """Rs.resample_array(x, rate, chunk) through run_rs: the outputs alone."""
    return run_rs(api, r, x, rate, cuts=chunk, **kw)[0]


def fir_filter(api, f, x, **kw):
    """Fir.filter(x) through run_fir."""
    return run_fir(api, f, x, **kw)


# ------------------------------------------------------------------------------------------------ the measurement blocks
# run_psd / run_corr / run_iir: the calls Psd / Corr / Iir.process_stream make, every stream of the input at an offset inside
# a buffer of poison with in_stride > n_in, every output poisoned before EVERY call with a front guard, gaps between its
# rows and a tail guard, every stride greater than its payload.  After each call every buffer is read back whole:
# check_written with cap == k (none of the three contracts grants slack: include/sfe_dsp.h names exactly what a call
# writes), then check_input_intact.  Counts are closed forms, checked before the bytes; a wrong one raises CountError.
def _odd_stride(n_items, item, unit, gap):
    """The smallest stride (items) >= n_items + gap whose bytes are an ODD multiple of `unit` bytes."""
    s = n_items + gap
    while (s * item) % unit or ((s * item) // unit) % 2 == 0:
        s += 1
    return s


def measure_strides(n_in, in_item, n_out, out_item, aligned=True):
    """(in_stride, out_stride) in items: both greater than their payloads, different from one another where the items are
    the same size, odd multiples of 16 bytes (aligned) or odd counts of items (else)."""
    si = _odd_stride(n_in, in_item, 16 if aligned else in_item, 7)
    so = _odd_stride(n_out, out_item, 16 if aligned else out_item, 5)
    if si == so:
        si = _odd_stride(n_in, in_item, 16 if aligned else in_item, si - n_in + 1)
    return si, so


def _measure_input(x, nch, item, a, b, aligned, stride):
    """_lay_input at a stride of the caller's: front 64 bytes, one item more when not aligned (cf32 8 bytes, u8 2 bytes, a
    real stream 4 bytes past a 16-byte boundary)."""
    lay = Layout(nch, item, b - a, stride, 64 + (0 if aligned else item), 64, 4)
    raw = lay.poisoned()
    rows = np.ascontiguousarray(x).reshape(nch, -1).view(np.uint8)
    for c in range(nch):
        lay.put(raw, c, rows[c, a * item:b * item])
    return lay, raw


def _measure_x(h, x, in_u8, w):
    nch = h.n_streams
    x = np.ascontiguousarray(x, dtype=np.uint8 if in_u8 else np.float32 if w == 1 else np.complex64).reshape(nch, -1)
    item = 2 if in_u8 else 4 * w
    return x, item, x.view(np.uint8).shape[1] // item


def psd_rows_of_call(segments_before, n_in, H, A):
    """include/sfe_dsp.h: *n_rows = floor((segments_before mod A + n_in / H) / A)."""
    return (segments_before % A + n_in // H) // A


def run_psd(api, ps, x, cuts=None, in_u8=False, aligned=True, segments_before=None, strides=None):
    """Psd.process_stream through poisoned, guarded buffers: x (n_streams, n) complex64 -- (n_streams, 2n) uint8 with in_u8
    -- fed in the calls [cuts[i], cuts[i+1]) (samples, multiples of hop).  The runner counts the segments itself (from
    `segments_before`, else from what earlier run_psd calls on this handle left, else 0; after a reset pass 0) and holds every call to
    rows = floor((segments_before mod A + n_in/H) / A).  A call that completes no row must leave its whole output buffer
    (room for a row per stream, and the guards) poison.  Returns ((n_streams, rows, N) float32, the per-call counts)."""
    S, N, H, A = ps.n_streams, ps.n_fft, ps.hop, ps.n_avg
    x, item, n = _measure_x(ps, x, in_u8, 2)
    cuts = _cuts(cuts, n)
    seen = int(getattr(ps, "_segments_seen", 0) if segments_before is None else segments_before)
    outs, counts = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        m = b - a
        assert m % H == 0 and m > 0
        want = psd_rows_of_call(seen, m, H, A)
        si, so = strides(m, want * N) if strides else measure_strides(m, item, want * N, 4, aligned)
        ilay, iraw = _measure_input(x, S, item, a, b, aligned, si)
        # no row due: the declared range is empty, and a row stored by mistake for any stream still lands in the tail guard
        olay = Layout(S, 4, want * N, so, 256, 256 + (0 if want else 4 * N))
        d_in, d_out = _upload(api, iraw), _upload(api, olay.poisoned())
        try:
            k = ps.process_stream(d_in.ptr + ilay.front, m, d_out.ptr + olay.front, in_stride=si, out_stride=so)
            oraw, iafter = _download(d_out), _download(d_in)
        finally:
            d_in.free()
            d_out.free()
        seen += m // H
        ps._segments_seen = seen
        if k != want:
            raise CountError("call [%d, %d): %d rows, floor((%d mod %d + %d) / %d) = %d" % (a, b, k, seen - m // H, A, m // H, A, want))
        check_written(oraw, olay, want * N)
        check_input_intact(iafter, iraw)
        counts.append(k)
        outs.append(np.stack([olay.take(oraw, s, want * N) for s in range(S)]).reshape(S, want, N))
    y = np.concatenate(outs, axis=1) if outs else np.zeros((S, 0, N), np.float32)
    return y, counts


def run_corr(api, cr, x, cuts=None, in_u8=False, aligned=True, dense=True, strides=None):
    """Corr.process_stream through poisoned, guarded buffers: x (n_streams, n) complex64 -- (n_streams, 2n) uint8 with in_u8
    -- fed in the calls [cuts[i], cuts[i+1]) (samples, multiples of block).  peak_val, peak_idx and (dense) the metric each
    sit in a buffer of their own with a front guard, gaps between the (stream, template) rows and a tail guard; exactly
    n_in / B cells per row of each peak array and n_in per row of the metric lose their poison.  Returns (peak_val
    (n_streams, K, blocks) float32, peak_idx uint32, m (n_streams, K, n) float32 or None, the per-call block counts)."""
    S, K, B = cr.n_streams, cr.n_templates, cr.block
    x, item, n = _measure_x(cr, x, in_u8, 2)
    cuts = _cuts(cuts, n)
    vals, idxs, ms, counts = [], [], [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        m = b - a
        assert m % B == 0 and m > 0
        want = m // B
        si, sp = strides(m, want) if strides else measure_strides(m, item, want, 4, aligned)
        sm = _odd_stride(m, 4, 16 if aligned else 4, 9)
        ilay, iraw = _measure_input(x, S, item, a, b, aligned, si)
        play = Layout(S * K, 4, want, sp, 256, 256)
        mlay = Layout(S * K, 4, m, sm, 256, 256)
        d_in, d_val, d_idx = _upload(api, iraw), _upload(api, play.poisoned()), _upload(api, play.poisoned())
        d_m = _upload(api, mlay.poisoned()) if dense else None
        try:
            k = cr.process_stream(d_in.ptr + ilay.front, m, d_val.ptr + play.front, d_idx.ptr + play.front,
                                  d_m.ptr + mlay.front if dense else None, in_stride=si, peak_stride=sp, metric_stride=sm)
            vraw, xraw, iafter = _download(d_val), _download(d_idx), _download(d_in)
            mraw = _download(d_m) if dense else None
        finally:
            for d in (d_in, d_val, d_idx, d_m):
                if d is not None:
                    d.free()
        if k != want:
            raise CountError("call [%d, %d): %d blocks, n_in / B = %d" % (a, b, k, want))
        check_written(vraw, play, want)
        check_written(xraw, play, want)
        if dense:
            check_written(mraw, mlay, m)
        check_input_intact(iafter, iraw)
        counts.append(k)
        vals.append(np.stack([play.take(vraw, r, want) for r in range(S * K)]).reshape(S, K, want))
        idxs.append(np.stack([play.take(xraw, r, want, np.uint32) for r in range(S * K)]).reshape(S, K, want))
        if dense:
            ms.append(np.stack([mlay.take(mraw, r, m) for r in range(S * K)]).reshape(S, K, m))
    return np.concatenate(vals, axis=2), np.concatenate(idxs, axis=2), np.concatenate(ms, axis=2) if dense else None, counts


def run_iir(api, f, x, cuts=None, in_u8=False, aligned=True, strides=None):
    """Iir.process_stream through poisoned, guarded buffers: x (n_streams, n) complex64 -- float32 on a real handle,
    (n_streams, 2n) uint8 with in_u8 -- fed in the calls [cuts[i], cuts[i+1]) (samples, multiples of the block).  strides:
    a function (n_in, n_out) -> (in_stride, out_stride) in items, else measure_strides.  n_out == n_in, or CountError.
    Returns (n_streams, n) complex64 / float32."""
    S, w = f.n_streams, 2 if f.data_complex else 1
    x, item, n = _measure_x(f, x, in_u8, w)
    cuts = _cuts(cuts, n)
    outs = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        m = b - a
        assert m > 0
        si, so = strides(m, m) if strides else measure_strides(m, item, m, 4 * w, aligned)
        ilay, iraw = _measure_input(x, S, item, a, b, aligned, si)
        olay = Layout(S, 4 * w, m, so, 256, 256)
        d_in, d_out = _upload(api, iraw), _upload(api, olay.poisoned())
        try:
            k = f.process_stream(d_in.ptr + ilay.front, m, d_out.ptr + olay.front, in_stride=si, out_stride=so)
            oraw, iafter = _download(d_out), _download(d_in)
        finally:
            d_in.free()
            d_out.free()
        if k != m:
            raise CountError("call [%d, %d): n_out %d, n_in %d" % (a, b, k, m))
        check_written(oraw, olay, m)
        check_input_intact(iafter, iraw)
        outs.append(np.stack([olay.take(oraw, s, m, np.complex64 if w == 2 else np.float32) for s in range(S)]))
    return np.concatenate(outs, axis=1)


# ------------------------------------------------------------------------------------------------ guarded buffers in place
# For tests that keep buffers of their own (device-resident streams, outputs laid one behind the other, strides and
# offsets of their choosing): api.DeviceArray's interface, with a guard of poison on either side of the body and the
# body poisoned (an output) or uploaded (an input).  `ptr` is the body, 256 bytes behind the allocation's start, so the
# test's own pointer arithmetic keeps its alignment.  An output's floats are poisoned again once they have been read
# back, so a later call that fails to store them cannot hand back the earlier call's values.  check_guarded() -- from an
# autouse fixture of the test module -- holds every guard to the poison and every input to what was uploaded.
GUARD_FLOATS = 64
_live = []


class Guarded:
    def __init__(self, api, n_floats, body=None):
        self._api, self.n = api, int(n_floats)
        self._d = api.DeviceArray(self.n + 2 * GUARD_FLOATS)
        self._L = self._d._L
        raw = np.full(self.n + 2 * GUARD_FLOATS, POISON, dtype=np.uint32)
        self.is_input = body is not None
        if body is not None:
            b = np.ascontiguousarray(body).reshape(-1).view(np.uint8)
            raw.view(np.uint8)[4 * GUARD_FLOATS:4 * GUARD_FLOATS + b.size] = b
        self._put(raw, 0)
        self._uploaded = raw if body is not None else None
        self.ptr = self._d.ptr + 4 * GUARD_FLOATS
        _live.append(self)

    def _put(self, raw, at_float):
        raw = np.ascontiguousarray(raw)
        self._api.check(self._L.sfe_dsp_memcpy_h2d(self._d.ptr + 4 * at_float, raw.ctypes.data, raw.nbytes, None))
        self._api.check(self._L.sfe_dsp_sync(None))

    def __int__(self):
        return self.ptr

    __index__ = __int__

    def to_numpy(self, n_floats=None, offset=0, stream=None, keep=False):
        """keep: leave an output's floats in place (a test that reads them again to see that a later call left them alone)"""
        n = self.n - offset if n_floats is None else int(n_floats)
        assert 0 <= offset and offset + n <= self.n, "a read outside the body"
        out = self._d.to_numpy(n, offset=GUARD_FLOATS + int(offset), stream=stream)
        if not self.is_input and not keep and n:
            self._put(np.full(n, POISON, dtype=np.uint32), GUARD_FLOATS + int(offset))
        return out

    def fill_synth(self, seed, channel=0, first=0, n_floats=None, offset=0, stream=None):
        self.is_input, self._uploaded = True, None
        n = self.n - offset if n_floats is None else int(n_floats)
        self._api.check(self._L.sfe_dsp_synth_fill(self.ptr + 4 * int(offset), n, seed, channel, first, stream))

    def zero(self, stream=None):
        self.is_input, self._uploaded = True, None          # the test wants to see zeros where nothing is stored: no re-poisoning
        self._api.check(self._L.sfe_dsp_memset(self.ptr, 0, self.n * 4, stream))

    def check(self):
        if getattr(self._d, "ptr", None) is None:
            return
        raw = self._d.to_numpy().view(np.uint32)
        for name, g in (("front", raw[:GUARD_FLOATS]), ("tail", raw[GUARD_FLOATS + self.n:])):
            if (g != POISON).any():
                raise WrittenError("a store in the %s guard of a %d-float buffer, word %d" % (name, self.n, int(np.flatnonzero(g != POISON)[0])))
        if self._uploaded is not None:
            check_input_intact(raw, self._uploaded)

    def free(self):
        if getattr(self._d, "ptr", None) is not None:
            try:
                self.check()
            finally:
                self._d.free()
                if self in _live:
                    _live.remove(self)
                self.ptr = None


def device_array(api, n_floats):
    """api.DeviceArray(n_floats), poisoned and guarded."""
    return Guarded(api, n_floats)


def from_numpy(api, a):
    """api.DeviceArray.from_numpy(a) between guards, held to its contents."""
    a = np.ascontiguousarray(a, dtype=np.float32).ravel()
    return Guarded(api, a.size, a)


def from_bytes(api, b):
    """api.DeviceArray.from_bytes(b) between guards (the bytes, then poison), held to its contents."""
    b = np.ascontiguousarray(b, dtype=np.uint8).ravel()
    return Guarded(api, (b.size + 3) // 4 + 4, b)


def check_guarded():
    """Every guarded buffer still alive: guards intact, inputs unchanged.  Then they are released."""
    live, errors = list(_live), []
    del _live[:]
    for g in live:
        try:
            g.check()
        except AssertionError as e:           # judge them all, free them all
            errors.append(e)
        finally:
            g._d.free()
            g.ptr = None
    if errors:
        raise errors[0]
