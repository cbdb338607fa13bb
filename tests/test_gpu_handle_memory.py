"""Device memory comes back when the FIR, resampler and pipe handles are destroyed.  Needs a real MI355X: run with `-m gpu`.

Through the public C ABI only, each case runs create -> use -> destroy cycles: one warm-up cycle, a reading of the device's
free bytes (hipMemGetInfo), four more cycles, a second reading.  The drop must be at most 16 MiB.  Every buffer a case names
is sized, from the arguments the case passes, so that leaking it once per cycle costs well beyond that bound over four cycles
(16 MiB buffers: 64 MiB; the staging set of sfe_dsp_fir_process_host is fixed at 2^20 samples per chunk, 8 MiB for each of
its two device buffers: 32 MiB each).  The device-wide number also moves with what other processes on the device allocate, so
a case measures up to three times and passes when one measurement is within the bound: a leak is monotone and fails all
three, a neighbour does not.

What this cannot see: the small owners -- the 16 KiB work counters, the twiddle and spectrum tables, events, streams -- are
below the bound.  They are covered by every free in csrc/ living inside an owner of block.h, and by review.  Outputs are
checked only for the counts the calls return; parity is the other tests' job.
"""
import ctypes as C

import numpy as np
import pytest

from simplefe_amd import synth

pytestmark = pytest.mark.gpu

MIB = 1 << 20
BOUND = 16 * MIB
CYCLES = 4
ROUNDS = 3


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    assert a.device_count() >= 1, "no GPU visible"
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMemGetInfo.argtypes, h.hipMemGetInfo.restype = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)], C.c_int
    return h


def _free_bytes(hip):
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def _memory_comes_back(hip, cycle):
    cycle()                                  # warm-up: what the runtime keeps for itself after the first use
    drops = []
    for _ in range(ROUNDS):
        before = _free_bytes(hip)
        for _ in range(CYCLES):
            cycle()
        drops.append(before - _free_bytes(hip))
        print("free bytes dropped by %d over %d cycles" % (drops[-1], CYCLES))
        if drops[-1] <= BOUND:
            return
    pytest.fail("device memory does not come back: %s bytes lost over %d cycles, three times" % (drops, CYCLES))


def test_multichannel_fir_history(api, L, hip):
    """256 taps: 256 cf32 samples of history per channel; 8192 channels make each of the two history buffers 16 MiB."""
    n_taps, n_channels = 256, 8192
    assert n_channels * 256 * 8 >= 16 * MIB
    taps = synth.lowpass_taps(n_taps, 0.2)

    def cycle():
        api.Fir(taps, data_complex=True, n_channels=n_channels).close()

    _memory_comes_back(hip, cycle)


def test_fir_host_staging(api, L, hip):
    """sfe_dsp_fir_process_host stages 2^20-sample chunks: 8 MiB of cf32 in each of the two device buffers (and pinned
    twins); 2^20 + 4096 samples take a full chunk through them and a short one behind it."""
    n = (1 << 20) + 4096
    assert (1 << 20) * 8 * CYCLES > BOUND
    taps = synth.taps_cfg2()
    x = synth.synth_cf32(n, ch=2)
    y = np.empty_like(x)
    lib = L.load()

    def cycle():
        f = api.Fir(taps, data_complex=True)
        api.check(lib.sfe_dsp_fir_process_host(f._h, x.ctypes.data, y.ctypes.data, n))
        f.close()

    _memory_comes_back(hip, cycle)


def test_fir_replan_for_tx10(api, L, hip):
    """3000 taps are planned as two partitions; 10-bit output re-plans the handle as one launch: new tables and a new history
    of 3072 cf32 samples per channel beside the old one; 704 channels make each history buffer 16.5 MiB."""
    n_taps, n_channels = 3000, 704
    ovl, parts = C.c_int(0), C.c_int(0)
    api.check(L.load().sfe_dsp_fir_plan(n_taps, C.byref(ovl), C.byref(parts), None))
    assert parts.value == 2 and n_channels * ((n_taps - 1 + 255) // 256 * 256) * 8 >= 16 * MIB
    taps = (synth.lowpass_taps(n_taps, 0.1) * 0.8).astype(np.float32)

    def cycle():
        f = api.Fir(taps, data_complex=True, n_channels=n_channels)
        f.set_output_format(L.FMT_TX10)
        f.close()

    _memory_comes_back(hip, cycle)


def test_rs_u8_conversion_scratch(api, L, hip):
    """u8 input at a step of 128, beyond the tiled kernels: the call's bytes are converted once into a float32 scratch of the
    handle, 16 MiB for 2^21 complex samples."""
    n, step = 1 << 21, 128
    assert n * 2 * 4 >= 16 * MIB
    taps = synth.lowpass_taps(32, 0.9 / step)
    d_in = api.DeviceArray.from_bytes(synth.offset_bytes(n, seed=synth.SEED + 3))
    cap = n // step + 8
    d_out = api.DeviceArray(2 * cap)

    def cycle():
        r = api.Rs(taps, 1, 4096, mode=L.RS_RESAMPLE, data_complex=True)
        r.set_input_format(L.FMT_U8)
        k = r.process_stream(d_in, n, d_out, cap, float(step))
        assert k == (n - 2) // step + 1
        r.close()

    _memory_comes_back(hip, cycle)
    d_in.free()
    d_out.free()


def test_fir_pipe_slots(api, L, hip):
    """A pipe of 2^21 cf32 items per batch: each of the four slots holds 16 MiB in each of its two device buffers (and pinned
    twins).  One batch pushed and pulled; the pipe is destroyed before the filter it borrows."""
    batch = 1 << 21
    assert batch * 8 >= 16 * MIB
    taps = synth.taps_cfg2()
    x = synth.synth_cf32(batch, ch=3)
    y = np.empty_like(x)
    lib = L.load()

    def cycle():
        f = api.Fir(taps, data_complex=True)
        p = C.c_void_p()
        api.check(lib.sfe_dsp_fir_pipe_create(f._h, batch, C.byref(p)))
        taken, got = C.c_size_t(0), C.c_size_t(0)
        api.check(lib.sfe_dsp_pipe_push(p, x.ctypes.data, batch, C.byref(taken)))
        assert taken.value == batch
        api.check(lib.sfe_dsp_pipe_pull(p, y.ctypes.data, batch, 2, C.byref(got)))
        assert got.value == batch
        assert lib.sfe_dsp_pipe_destroy(p) == L.SFE_OK
        assert lib.sfe_dsp_fir_destroy(f._h) == L.SFE_OK
        f._h = None

    _memory_comes_back(hip, cycle)
