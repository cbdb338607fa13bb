#!/usr/bin/env python3
"""The spatial covariance estimator (sfe_dsp_cov_*) over 2^28 input samples per call, generated in HBM by
sfe_dsp_synth_fill (u8: the first 2^29 bytes of the same buffer as (I,Q) pairs), one call per launch: HIP events,
12 warm-up calls (beyond the chip's post-idle transient) then 20 timed calls, mean.  Every call starts on a row: the
call is a whole number of rows.
    bytes = input once + output rows once
    flop  = 512 per instant, band and 16 x 16 tile ISSUED: NT (NT + 1) / 2 tiles, NT = ceil(S / 8) (the upper triangle)
    t_hbm = bytes / 6.29 TB/s (the measured copy ceiling);  t_fp32 = flop / 157.3 TFLOP/s;  frac = max of the two / time
Beside each row, the same law composed in torch-ROCm in the same process over the same device buffers: complex64
X @ X.mH per band and row, times 1/A (the u8 leg converting the bytes to complex64 first); warm-up then 5 timed calls.
The composition is checked against the block's first row of band 0 (C out of the Gram matrix).
    python scripts/time_cov.py > profiles/cov/time_cov.txt
LOG2N=24 shortens the stream; TORCH=0 leaves the torch composition out; SHAPES="S:M:A:fmt;..." limits the run to those
rows (A = 0: one row, the whole call)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api, lib, synth  # noqa: E402

WARM, REPS, TORCH_REPS = 12, 20, 5
TORCH = os.environ.get("TORCH", "1") != "0"
N_IN = 1 << int(os.environ.get("LOG2N", "28"))            # input samples per call, over all streams and bands
SHAPES = [(1, 1, 1 << 20), (4, 1, 4096), (8, 256, 64), (16, 1, 4096), (64, 1, 4096), (64, 1, 0)]      # A = 0: one row
WANT = {tuple(s.split(":")) for s in os.environ["SHAPES"].split(";")} if os.environ.get("SHAPES") else None
HBM_TBS, FP32_TFS = 6.29, 157.3


def time_calls(run, warm, reps):
    t = api.Timer()
    for _ in range(warm):
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


def torch_gram(torch, xi, S, M, rows, A, u8):
    """(M, rows, S, S) complex64: X X^H / A per band and row, X the (S, A) block of the row."""
    if u8:
        xi = torch.view_as_complex((xi.to(torch.float32) - 128.0) * (1.0 / 127.0))
    X = xi.reshape(S, M, rows, A).permute(1, 2, 0, 3)
    return torch.matmul(X, X.mH) * (1.0 / A)


def main():
    x = api.DeviceArray(2 * N_IN)
    x.fill_synth(synth.SEED)
    torch = None
    if TORCH:
        import torch
        print(f"# torch {torch.__version__}")
    print(f"# 2^{N_IN.bit_length() - 1} input samples per call over all streams and bands; floors: {HBM_TBS} TB/s, {FP32_TFS} TFLOP/s")
    print(f"{'S':>3s} {'M':>4s} {'A':>8s} {'in':>5s} {'n':>10s} {'ms':>8s} {'GB':>6s} {'GFLOP':>8s} {'t_hbm':>7s} {'t_fp32':>7s} {'frac':>6s} "
          f"{'torch ms':>9s} {'x':>6s}   check")
    for S, M, A0 in SHAPES:
        n = N_IN // (S * M)
        A = A0 or n
        if A > n or n % A:
            continue                                                # a shortened stream that holds no whole row
        rows, gram = n // A, 4 * S * S
        nt = -(-S // 8)
        for fmt in ("cf32", "u8"):
            if WANT is not None and (str(S), str(M), str(A0), fmt) not in WANT:
                continue
            u8 = fmt == "u8"
            cov = api.Cov(S, M, A, 1.0 / A)
            if u8:
                cov.set_input_format(lib.FMT_U8)
            y = api.DeviceArray(M * rows * gram)
            ms = time_calls(lambda: cov.process_stream(x, n, y), WARM, REPS)
            gb = ((2 if u8 else 8) * N_IN + 4.0 * M * rows * gram) / 1e9
            gf = 512.0 * (nt * (nt + 1) // 2) * M * n / 1e9
            t_hbm, t_fp = gb / HBM_TBS, gf / FP32_TFS               # ms: GB over TB/s, GFLOP over TFLOP/s
            note = f"{'':>9s} {'':>6s}"
            if torch is not None:
                api.sync()
                Cm, _ = synth.cov_from_gram(y.to_numpy(gram).reshape(2 * S, 2 * S))
                dev = torch.device("cuda:0")
                if u8:
                    xi = torch.as_tensor(_Cai(x.ptr, (S, M, n, 2), "|u1"), device=dev)
                else:
                    xi = torch.view_as_complex(torch.as_tensor(_Cai(x.ptr, (S, M, n, 2), "<f4"), device=dev))
                last = []

                def run():
                    last[:] = [torch_gram(torch, xi, S, M, rows, A, u8)]
                tm = time_calls(run, 2, TORCH_REPS)
                torch.cuda.synchronize()
                theirs = last[0][0, 0].cpu().numpy().astype(np.complex128)
                chk = np.abs(theirs - Cm).max() / np.abs(Cm).max()
                lost = "" if tm >= ms else "   SLOWER THAN TORCH"
                note = f"{tm:9.3f} {tm / ms:6.2f}   max |C - torch| / max |C| {chk:.1e}{lost}"
                del xi, last
                torch.cuda.empty_cache()
            cov.close()
            y.free()
            print(f"{S:3d} {M:4d} {A:8d} {fmt:>5s} {n:10d} {ms:8.3f} {gb:6.2f} {gf:8.1f} {t_hbm:7.3f} {t_fp:7.3f} {max(t_hbm, t_fp) / ms:6.3f} {note}",
                  flush=True)
    x.free()


if __name__ == "__main__":
    main()
