#!/usr/bin/env python3
"""The beamformer / stream-mixing bank (sfe_dsp_beam_*) over 2^28 input samples per call, generated in HBM by
sfe_dsp_synth_fill (u8: the first 2^29 bytes of the same buffer as (I,Q) pairs), one call per launch: HIP events,
warm-up then 20 timed calls, mean.  Weights: synth.beam_steering_weights (every band the same set), V absent.
    bytes = input once + output once;  flop = 8 S B per instant and band (a real 2B x 2S product)
    floor = max(bytes / 6.29 TB/s (the measured copy ceiling), flop / 157.3 TFLOP/s);  frac = floor / time
Beside each row, the same law composed in torch-ROCm in the same process over the same device buffers: complex64
matmul (bmm over the bands for M > 1, its output left band-major), the u8 leg converting the bytes to complex64 first;
warm-up then 5 timed calls.  The composition is checked against the block on a short stream first.
    python scripts/time_beam.py > profiles/beam/time_beam.txt
LOG2N=24 shortens the stream; TORCH=0 leaves the torch composition out; SHAPES="S:B:M:fmt;..." limits the run to those rows."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api, lib, synth  # noqa: E402

REPS, TORCH_REPS = 20, 5
TORCH = os.environ.get("TORCH", "1") != "0"
N_IN = 1 << int(os.environ.get("LOG2N", "28"))            # input samples per call, over all streams and bands
SHAPES = [(1, 1, 1), (4, 1, 1), (8, 8, 1), (16, 4, 1), (64, 8, 1), (64, 64, 1), (8, 8, 256)]
WANT = {tuple(s.split(":")) for s in os.environ["SHAPES"].split(";")} if os.environ.get("SHAPES") else None
HBM_TBS, FP32_TFS = 6.29, 157.3


def time_calls(run, reps):
    t = api.Timer()
    for _ in range(3):
        run()
    t.start()
    for _ in range(reps):
        run()
    t.stop()
    return t.elapsed_ms() / reps


class _Cai:
    """A window of a DeviceArray for torch.as_tensor (the CUDA array interface, which torch-ROCm reads too)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def torch_views(torch, x, y, S, B, M, n, u8):
    """(input (S, M, n) complex64 -- or (S, M, n, 2) uint8 --, output (M, B, n) complex64) over the buffers x, y."""
    dev = torch.device("cuda:0")
    if u8:
        xi = torch.as_tensor(_Cai(x.ptr, (S, M, n, 2), "|u1"), device=dev)
    else:
        xi = torch.view_as_complex(torch.as_tensor(_Cai(x.ptr, (S, M, n, 2), "<f4"), device=dev))
    yo = torch.view_as_complex(torch.as_tensor(_Cai(y.ptr, (M, B, n, 2), "<f4"), device=dev))
    return xi, yo


def torch_mix(torch, Wt, xi, yo, u8):
    if u8:
        xi = torch.view_as_complex((xi.to(torch.float32) - 128.0) * (1.0 / 127.0))
    if Wt.shape[0] == 1:
        torch.matmul(Wt[0], xi[:, 0], out=yo[0])
    else:
        torch.bmm(Wt, xi.permute(1, 0, 2), out=yo)


def main():
    x = api.DeviceArray(2 * N_IN)
    x.fill_synth(synth.SEED)
    out_floats = max(2 * N_IN // (S * M) * B * M for S, B, M in SHAPES)
    y = api.DeviceArray(out_floats)
    torch = None
    if TORCH:
        import torch
        print(f"# torch {torch.__version__}")
    print(f"# 2^{N_IN.bit_length() - 1} input samples per call over all streams and bands; floors: {HBM_TBS} TB/s, {FP32_TFS} TFLOP/s")
    print(f"{'S':>3s} {'B':>3s} {'M':>4s} {'in':>5s} {'n':>10s} {'ms':>8s} {'GB':>6s} {'GFLOP':>8s} {'bound':>5s} {'frac':>6s} {'torch ms':>9s} {'x':>6s}   check")
    for S, B, M in SHAPES:
        n = N_IN // (S * M)
        W = np.ascontiguousarray(np.broadcast_to(synth.beam_steering_weights(S, B), (M, B, S)))
        for fmt in ("cf32", "u8"):
            if WANT is not None and (str(S), str(B), str(M), fmt) not in WANT:
                continue
            u8 = fmt == "u8"
            beam = api.Beam(W)
            if u8:
                beam.set_input_format(lib.FMT_U8)
            ms = time_calls(lambda: beam.process_stream(x, n, y), REPS)
            gb = ((2 if u8 else 8) * N_IN + 8 * B * M * n) / 1e9
            gf = 8.0 * S * B * M * n / 1e9
            t_hbm, t_fp = gb / HBM_TBS, gf / FP32_TFS                   # ms: GB over TB/s, GFLOP over TFLOP/s
            floor, bound = max(t_hbm, t_fp), ("HBM" if t_hbm >= t_fp else "FP32")
            note = f"{'':>9s} {'':>6s}"
            if torch is not None:
                Wt = torch.from_numpy(W).to("cuda:0")
                m = min(n, 4096)                                        # the check: the first m samples of every row
                beam.process_stream(x, m, y, in_stride=n, out_stride=m)
                api.sync()
                mine = y.to_numpy(2 * B * M * m).view(np.complex64).reshape(B, M, m)
                xi, yo = torch_views(torch, x, y, S, B, M, n, u8)
                tm = time_calls(lambda: torch_mix(torch, Wt, xi, yo, u8), TORCH_REPS)
                torch.cuda.synchronize()
                theirs = np.ascontiguousarray(yo[:, :, :m].permute(1, 0, 2).cpu().numpy())
                chk = synth.rel_rms(theirs.view(np.float32), mine.view(np.float32))
                note = f"{tm:9.3f} {tm / ms:6.2f}   rel-RMS between the two {chk:.1e}"
                del xi, yo, Wt
                torch.cuda.empty_cache()
            beam.close()
            print(f"{S:3d} {B:3d} {M:4d} {fmt:>5s} {n:10d} {ms:8.3f} {gb:6.2f} {gf:8.1f} {bound:>5s} {floor / ms:6.3f} {note}", flush=True)
    x.free()
    y.free()


if __name__ == "__main__":
    main()
