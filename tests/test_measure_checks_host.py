"""Negative controls for run_psd / run_corr / run_iir of tests/stream_checks.py, on the CPU.  A fake `api` whose DeviceArray
is a host numpy buffer (its .ptr the buffer's real address) and fake handles with the process_stream signatures of
api.Psd, api.Corr and api.Iir, which compute the block's float64 reference (synth.psd_reference, synth.corr_reference,
synth.iir_reference) and store it through np.ctypeslib.as_array at the pointers and strides they are given.  Each runner
passes its honest fake, and raises the NAMED exception for each fault planted in the fake, one at a time."""
import ctypes as C
import types

import numpy as np
import pytest

import stream_checks as sc
from simplefe_amd import synth


# ------------------------------------------------------------------------------------------------ the fake api
class DeviceArray:
    def __init__(self, n_floats):
        self._a = np.zeros(int(n_floats), np.float32)
        self.n, self.ptr = self._a.size, self._a.ctypes.data

    @classmethod
    def from_numpy(cls, a):
        a = np.ascontiguousarray(a, dtype=np.float32).ravel()
        d = cls(a.size)
        d._a.view(np.uint32)[:] = a.view(np.uint32)        # bits, NaN payloads included
        return d

    def to_numpy(self):
        return self._a.copy()

    def free(self):
        self._a, self.ptr = None, None


API = types.SimpleNamespace(DeviceArray=DeviceArray)


def _mem(ptr, nbytes, dtype=np.uint8):
    return np.ctypeslib.as_array((C.c_uint8 * int(nbytes)).from_address(int(ptr))).view(dtype)


class _Fake:
    """What the three fakes share: the streams read so far, the planted fault, loads and stores at raw addresses."""

    def __init__(self, n_streams, in_u8=False, data_complex=True, fault=None):
        self.n_streams, self.in_u8, self.data_complex, self.fault = n_streams, in_u8, data_complex, fault
        self.item = 2 if in_u8 else 8 if data_complex else 4
        self.seen = [np.zeros(0, np.complex64 if data_complex else np.float32) for _ in range(n_streams)]

    def _read(self, d_in, n_in, in_stride):
        unit = 1 if self.fault == "stride in bytes" else self.item          # the wrong unit: bytes for samples
        for s in range(self.n_streams):
            b = _mem(d_in + s * in_stride * unit, n_in * self.item).copy()
            v = synth.u8_to_cf32(b) if self.in_u8 else b.view(self.seen[s].dtype)
            self.seen[s] = np.concatenate([self.seen[s], v])
        if self.fault == "input word":
            _mem(d_in + self.item * (n_in // 2), 4, np.uint32)[0] ^= 1

    def _store(self, ptr, values):
        v = np.ascontiguousarray(values)
        _mem(ptr, v.nbytes)[:] = v.view(np.uint8).ravel()

    def _stray(self, d_out, payload_bytes):
        """The two faults that are one float stored outside the declared range."""
        if self.fault == "gap after stream 0":
            self._store(d_out + payload_bytes, np.float32([1.5]))
        if self.fault == "front guard":
            self._store(d_out - 4, np.float32([1.5]))


class FakePsd(_Fake):
    def __init__(self, window, hop, n_avg, scale=1.0, n_streams=1, **kw):
        super().__init__(n_streams, **kw)
        self.w = np.asarray(window, np.float32)
        self.n_fft, self.hop, self.n_avg, self.scale, self.rows_out = self.w.size, hop, n_avg, scale, 0

    def process_stream(self, d_in, n_in, d_out, in_stride=None, out_stride=None, stream=None):
        N = self.n_fft
        self._read(d_in, n_in, in_stride)
        total = (self.seen[0].size // self.hop) // self.n_avg
        k = total - self.rows_out
        for s in range(self.n_streams):
            rows = synth.psd_reference(self.seen[s], self.w, self.hop, self.n_avg, np.float32(self.scale))[self.rows_out:].astype(np.float32)
            flat = rows.ravel()
            if self.fault == "last left unstored" and s == self.n_streams - 1:
                flat = flat[:-1]
            self._store(d_out + 4 * s * out_stride, flat)
        self.rows_out = total
        if k:
            self._stray(d_out, 4 * k * N)
        elif self.fault == "a store with no row due":
            self._store(d_out, np.float32([1.5]))
        return k - 1 if self.fault == "count one short" and k else k


class FakeCorr(_Fake):
    def __init__(self, templates, block, min_energy=0.0, n_streams=1, **kw):
        super().__init__(n_streams, **kw)
        self.t = np.atleast_2d(np.asarray(templates, np.complex64))
        self.n_templates, self.len, self.block, self.gate = self.t.shape[0], self.t.shape[1], block, min_energy

    def process_stream(self, d_in, n_in, d_peak_val, d_peak_idx, d_metric=None, in_stride=None, peak_stride=None, metric_stride=None,
                       stream=None):
        K, B = self.n_templates, self.block
        nb = n_in // B
        self._read(d_in, n_in, in_stride)
        for s in range(self.n_streams):
            m, val, idx = synth.corr_reference(self.seen[s], self.t, B, self.gate)
            for k in range(K):
                short = self.fault == "last left unstored" and s == self.n_streams - 1 and k == K - 1
                self._store(d_peak_val + 4 * (s * K + k) * peak_stride, val[k, -nb:].astype(np.float32)[:nb - short])
                self._store(d_peak_idx + 4 * (s * K + k) * peak_stride, idx[k, -nb:].astype(np.uint32))
                if d_metric is not None:
                    self._store(d_metric + 4 * (s * K + k) * metric_stride, m[k, -n_in:].astype(np.float32))
        self._stray(d_peak_val, 4 * nb)
        return nb - 1 if self.fault == "count one short" else nb


class FakeIir(_Fake):
    block = 64

    def __init__(self, sos, data_complex=True, n_streams=1, **kw):
        super().__init__(n_streams, data_complex=data_complex, **kw)
        self.sos = sos

    def process_stream(self, d_in, n_in, d_out, in_stride=None, out_stride=None, stream=None):
        self._read(d_in, n_in, in_stride)
        osz = 8 if self.data_complex else 4
        for s in range(self.n_streams):
            y = synth.iir_reference(self.seen[s], self.sos)[-n_in:].astype(self.seen[s].dtype)
            if self.fault == "last left unstored" and s == self.n_streams - 1:
                y = y[:-1]
            self._store(d_out + osz * s * out_stride, y)
        self._stray(d_out, osz * n_in)
        return n_in - 1 if self.fault == "count one short" else n_in


# ------------------------------------------------------------------------------------------------ the cases
S = 3
FMT = ["cf32", "u8"]
LAYOUTS = [True, False]
N, H, A = 256, 97, 2
PSD_CUTS = [0, 1 * H, 3 * H, 6 * H, 7 * H, 9 * H]          # 1, 2, 3, 1, 2 segments: the first call completes no row
W = np.hanning(N).astype(np.float32)
LT, KT = 13, 2
BT = 4096 - 256
SOS = synth.iir_dc_blocker(0.99)


def _input(fmt, n, real=False):
    if fmt == "u8":
        return np.stack([synth.offset_bytes(n, seed=7 + s) for s in range(S)])
    if real:
        return np.stack([synth.synth_f32(n, ch=20 + s) for s in range(S)])
    return np.stack([synth.synth_cf32(n, ch=20 + s).view(np.complex64) for s in range(S)])


def _samples(fmt, x):
    return np.stack([synth.u8_to_cf32(r) for r in x]) if fmt == "u8" else x


def _psd(fmt, aligned, fault=None):
    x = _input(fmt, PSD_CUTS[-1])
    y, counts = sc.run_psd(API, FakePsd(W, H, A, 0.37, S, in_u8=fmt == "u8", fault=fault), x, PSD_CUTS, in_u8=fmt == "u8", aligned=aligned)
    assert counts == [0, 1, 2, 0, 1]
    xs = _samples(fmt, x)
    for s in range(S):
        sc.check_values(y[s], synth.psd_reference(xs[s], W, H, A, np.float32(0.37)).astype(np.float32), exact=True, label="psd stream %d" % s)


def _templates():
    t = np.stack([synth.synth_cf32(LT, ch=100 + k).view(np.complex64) for k in range(KT)])
    return (np.sign(t.real) + 1j * np.sign(t.imag)).astype(np.complex64)


def _corr(fmt, aligned, fault=None, dense=True):
    x = _input(fmt, 4 * BT)
    t = _templates()
    val, idx, m, counts = sc.run_corr(API, FakeCorr(t, BT, 1e-6, S, in_u8=fmt == "u8", fault=fault), x, [0, BT, 3 * BT, 4 * BT],
                                      in_u8=fmt == "u8", aligned=aligned, dense=dense)
    assert counts == [1, 2, 1] and idx.dtype == np.uint32 and (m is None) == (not dense)
    xs = _samples(fmt, x)
    for s in range(S):
        rm, rv, ri = synth.corr_reference(xs[s], t, BT, 1e-6)
        sc.check_values(val[s], rv.astype(np.float32), exact=True, label="corr peak_val stream %d" % s)
        if not np.array_equal(idx[s], ri.astype(np.uint32)):
            raise sc.ValuesError("exact", "corr peak_idx stream %d" % s)
        if dense:
            sc.check_values(m[s], rm.astype(np.float32), exact=True, label="corr dense stream %d" % s)


def _iir(fmt, aligned, fault=None):
    real = fmt == "real"
    G = FakeIir.block
    x = _input(fmt, 4 * G, real)
    y = sc.run_iir(API, FakeIir(SOS, not real, S, in_u8=fmt == "u8", fault=fault), x, [0, G, 3 * G, 4 * G], in_u8=fmt == "u8", aligned=aligned)
    xs = _samples(fmt, x)
    assert y.shape == xs.shape and y.dtype == xs.dtype
    ref = synth.iir_reference(xs, SOS).astype(xs.dtype)
    sc.check_values(y.view(np.float32), ref.view(np.float32), exact=True, label="iir")


RUN = {"psd": _psd, "corr": _corr, "iir": _iir}
BLOCKS = [(b, f) for b in RUN for f in FMT + (["real"] if b == "iir" else [])]


# ------------------------------------------------------------------------------------------------ the controls
@pytest.mark.parametrize("aligned", LAYOUTS)
@pytest.mark.parametrize("block, fmt", BLOCKS)
def test_the_runners_pass_the_honest_fakes(block, fmt, aligned):
    RUN[block](fmt, aligned)


def test_the_layouts_are_what_the_runners_promise():
    for aligned in LAYOUTS:
        for n, item, out_item in ((3 * 1024, 8, 8), (3 * 1024, 2, 8), (1024, 4, 4), (5 * 97, 8, 4), (3840, 2, 4)):
            si, so = sc.measure_strides(n, item, n, out_item, aligned)
            assert si > n and so > n and si != so
            unit_i, unit_o = (16, 16) if aligned else (item, out_item)
            assert (si * item) % unit_i == 0 and (si * item // unit_i) % 2 == 1
            assert (so * out_item) % unit_o == 0 and (so * out_item // unit_o) % 2 == 1
            x = np.zeros((2, n * item), np.uint8)
            lay, raw = sc._measure_input(x, 2, item, 0, n, aligned, si)
            assert lay.front % 16 == (0 if aligned else item) and lay.stride_items == si
            owned = np.zeros(lay.total, bool)
            for c in range(2):
                owned[lay.start(c):lay.start(c) + lay.cap] = True
            assert sc._same_as_poison(raw)[~owned].all() and not raw.view(np.uint8)[owned].any()     # poison all around the samples


def test_dense_off_leaves_no_metric():
    _corr("cf32", True, dense=False)


@pytest.mark.parametrize("block, fmt", BLOCKS)
def test_one_float_in_the_gap_after_stream_0(block, fmt):
    with pytest.raises(sc.WrittenError, match="the gap after channel 0"):
        RUN[block](fmt, True, "gap after stream 0")


@pytest.mark.parametrize("block, fmt", BLOCKS)
def test_one_float_in_the_front_guard(block, fmt):
    with pytest.raises(sc.WrittenError, match="the front guard"):
        RUN[block](fmt, True, "front guard")


@pytest.mark.parametrize("block, fmt", BLOCKS)
def test_the_last_row_sample_or_block_left_unstored(block, fmt):
    with pytest.raises(sc.WrittenError, match="never stored"):
        RUN[block](fmt, False, "last left unstored")


@pytest.mark.parametrize("aligned", LAYOUTS)
@pytest.mark.parametrize("block, fmt", BLOCKS)
def test_one_input_word_changed(block, fmt, aligned):
    with pytest.raises(sc.InputError):
        RUN[block](fmt, aligned, "input word")


@pytest.mark.parametrize("block, fmt", BLOCKS)
def test_a_count_one_short(block, fmt):
    with pytest.raises(sc.CountError):
        RUN[block](fmt, True, "count one short")


@pytest.mark.parametrize("fmt", FMT)
def test_a_psd_call_with_no_row_due_that_stores_one_float(fmt):
    with pytest.raises(sc.WrittenError, match="outside the declared range"):
        _psd(fmt, True, "a store with no row due")


@pytest.mark.parametrize("aligned", LAYOUTS)
@pytest.mark.parametrize("block", list(RUN))
def test_a_stride_in_bytes_for_samples_on_u8(block, aligned):
    """The fake takes in_stride in bytes where it is in (I,Q) pairs: streams 1 and 2 are read from the wrong place.  The
    runner's own checks cannot see a wrong READ; the caller's comparison with the reference does (or, where poison bytes
    reach the output, nothing finite is left to compare)."""
    with pytest.raises((sc.WrittenError, sc.ValuesError)):
        RUN[block]("u8", aligned, "stride in bytes")


def test_the_psd_runner_counts_segments_itself():
    assert [sc.psd_rows_of_call(b, n, 97, 5) for b, n in ((0, 4 * 97), (4, 97), (5, 9 * 97), (14, 97), (15, 97))] == [0, 1, 1, 1, 0]
    x = _input("cf32", 6 * H)
    ps = FakePsd(W, H, A, 1.0, S)
    assert sc.run_psd(API, ps, x[:, :3 * H])[1] == [1]
    assert sc.run_psd(API, ps, x[:, 3 * H:])[1] == [2]             # the open segment of the first call counts
    with pytest.raises(sc.CountError):
        sc.run_psd(API, FakePsd(W, H, A, 1.0, S), x[:, :3 * H], segments_before=1)
