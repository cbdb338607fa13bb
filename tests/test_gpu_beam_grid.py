"""Every class of the beamformer's kernel (csrc/beam.hip: beam_kernel<KP, RT, U8>, KP in 1, 2, 4, 8, 16 pairs of K-steps,
RT in 1, 2, 4, 8 row tiles, cf32 and u8: 40 instantiations) on the GPU against float64, and the second pass of its
grid-stride loop.  `-m gpu`.

One test per class (KP, RT).  Each class has its own register tile (x[KP][NB], acc[RT][NB]), its own NB (2 column blocks
per tile where KP = 16 or RT = 8, else 4) and its own skip conditions (4p >= S, 8rt >= B, s < S, b >= B), so each runs at
the four corners of its range: S in {1..4, 5..8, 9..16, 17..32, 33..64} and B in {1..8, 9..16, 17..32, 33..64}, lower
and upper edge of both -- at the lower edges the most padding (KP = 4 at S = 9: one stream in the third K-step pair, the
fourth pair skipped; RT >= 2 at the smallest B of its range), at the upper edges none.  M = 2 bands, W and V both present,
both input formats, n in {1, 63, 65, 257}: 257 is one sample beyond what a workgroup's four waves hold at NB = 4.  Every
call goes through test_gpu_beam._guarded (input rows one sample into NaN patterns, 0xFF for u8, with in_stride > n; output
rows inside a sentinel with out_stride > n) and every output float is held to test_gpu_beam._check: the derived bound
2 (2S + 1) 2^-24 sum |R||x| and rel-RMS <= 1e-5, unchanged.  No tolerance is new.

The grid-stride case: the grid is capped at ceil(CUs per_cu / M) workgroups of four tiles, and no other test has more
tiles than that.  With M = 512 bands and n = 1100 there are 18 tiles (NB = 4) or 35 (NB = 2) per band; 8 is the most
workgroups of 256 threads a CU holds, so with tiles > 4 ceil(8 CUs / M), asserted before the call, the loop takes a
second pass whatever the occupancy query returned."""
import numpy as np
import pytest

import test_gpu_beam as tb
from simplefe_amd import synth

pytestmark = pytest.mark.gpu
S_RANGE = {1: (1, 4), 2: (5, 8), 4: (9, 16), 8: (17, 32), 16: (33, 64)}     # KP: S_lo, S_hi
B_RANGE = {1: (1, 8), 2: (9, 16), 4: (17, 32), 8: (33, 64)}                 # RT: B_lo, B_hi
CLASSES = {(kp, rt): [(s, b) for s in S_RANGE[kp] for b in B_RANGE[rt]] for kp in S_RANGE for rt in B_RANGE}
SIZES = [1, 63, 65, 257]
NMAX = max(SIZES)
M = 2
STRIDE_SHAPES = [(2, 2), (33, 1)]
STRIDE_M, STRIDE_N = 512, 1100


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


@pytest.mark.parametrize("cls", list(CLASSES), ids=lambda c: "KP%d-RT%d" % c)
def test_every_class_at_the_corners_of_its_range(api, L, cls):
    for S, B in CLASSES[cls]:
        W, V = tb._weights(S, B, M, 300 * S + B), tb._weights(S, B, M, 11 + 300 * S + B)
        beam = api.Beam(W, V)
        R = api.beam_plan(W, V)
        for u8 in (False, True):
            beam.set_input_format(L.FMT_U8 if u8 else L.FMT_F32)
            up, x = tb._input(S, M, NMAX, u8)
            ref, bound = synth.beam_reference(x, W, V), tb._bound(R, x)
            for n in SIZES:
                got, intact = tb._guarded(api, beam, np.ascontiguousarray(up[:, :, :(2 if u8 else 1) * n]), n, u8,
                                          extra_in=3, extra_out=5, shift_in=1)
                tag = "KP=%d RT=%d S=%d B=%d n=%d %s" % (cls + (S, B, n, "u8" if u8 else "cf32"))
                assert intact, tag
                tb._check(tag, got, ref[:, :, :n], bound[:, :, :n])
        beam.close()


def _cu_count():
    """The compute units of device 0, by the attribute beam.hip's launcher sizes its grid with (common.h:
    device_cu_count): hipDeviceAttributeMultiprocessorCount, 63 in hip_runtime_api.h's enumeration."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    hip.hipDeviceGetAttribute.argtypes, hip.hipDeviceGetAttribute.restype = [C.POINTER(C.c_int), C.c_int, C.c_int], C.c_int
    v = C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(v), 63, 0) == 0
    return v.value


def test_the_second_pass_of_the_grid_stride_loop(api, L):
    Mb, n = STRIDE_M, STRIDE_N
    cus = _cu_count()
    assert 16 <= cus <= 1024, cus                               # a count of compute units, not some other attribute
    for S, B in STRIDE_SHAPES:
        nb = 2 if S > 32 or B > 32 else 4                       # beam.hip: beam_nb
        tiles = -(-n // (16 * nb))
        assert tiles > 4 * -(-cus * 8 // Mb), (S, B, cus, tiles)        # more tiles than the largest grid's first pass
        W, V = tb._weights(S, B, Mb, 500 + S), tb._weights(S, B, Mb, 600 + S)
        beam = api.Beam(W, V)
        beam.set_input_format(L.FMT_U8)
        R = api.beam_plan(W, V)
        up = synth.offset_bytes(S * Mb * n, seed=synth.SEED + 13 * S + B).reshape(S, Mb, 2 * n)
        # plain buffers (16896 guarded rows would cost more host time than the case is worth): the output lies in a
        # sentinel with out_stride = n + 5, so every gap and the tail show a store of the second pass that went astray
        stride = n + 5
        image = np.full(B * Mb * stride * 2 + 64, tb.SENT, np.float32)
        d_in, d_out = api.DeviceArray.from_bytes(up), api.DeviceArray.from_numpy(image)
        try:
            assert beam.process_stream(d_in, n, d_out, out_stride=stride) == n
            out = d_out.to_numpy()
        finally:
            d_in.free()
            d_out.free()
            beam.close()
        body = out[:B * Mb * stride * 2].reshape(B, Mb, stride, 2)
        assert (tb._bits(body[:, :, n:]) == tb._bits(tb.SENT)).all() and (tb._bits(out[B * Mb * stride * 2:]) == tb._bits(tb.SENT)).all(), (S, B)
        got = np.ascontiguousarray(body[:, :, :n]).view(np.complex64)[..., 0]
        step = 64                                               # bands per slice: the float64 arrays stay below 100 MB
        for k0 in range(0, Mb, step):
            k1 = min(Mb, k0 + step)
            x = synth.u8_to_cf32(np.ascontiguousarray(up[:, k0:k1]).reshape(-1)).reshape(S, k1 - k0, n)
            tb._check("second pass S=%d B=%d bands %d..%d of %d, %d tiles, %d CUs" % (S, B, k0, k1 - 1, Mb, tiles, cus), got[:, k0:k1],
                      synth.beam_reference(x, W[k0:k1], V[k0:k1]), tb._bound(R[k0:k1], x))
