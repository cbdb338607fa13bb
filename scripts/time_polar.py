#!/usr/bin/env python3
"""The FM, phase and envelope detector (sfe_dsp_polar_*) over 2^28 samples per call, generated in HBM by
sfe_dsp_synth_fill (u8: the first bytes of the same buffer as (I,Q) pairs): one stream of 2^28 and 64 streams of 2^22, the
three modes, cf32 and u8.  Beside every row, on a torch tensor that holds the same bytes:
  copy   a bare kernel that moves the same bytes: torch's strided copy of the real parts (reads every 8-byte sample's line,
         writes 4 bytes per sample); for u8 its converting copy of the I bytes (2 bytes read per sample, 4 written);
  torch  what a user would have written: torch.angle(x[1:] * x[:-1].conj()) * g (FM, four launches), torch.angle(x) * g,
         torch.abs(x) * g; for u8 behind the conversion (b - 128) * (1/127).  It is held to the block within 1e-6 rad
         (AM: 1e-6 of the largest value) over the first CHECK samples of every stream before anything is timed.
Times: device events around WINDOW consecutive calls behind a warm-up, the three contenders' windows alternating, the median
of ROUNDS windows each.  frac = bytes / time / 6.29 TB/s (the measured copy ceiling), bytes = 12 (cf32) or 6 (u8) per sample.
    python scripts/time_polar.py > profiles/polar/time_polar.txt
LOG2N=22 shortens the call."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api, lib, synth  # noqa: E402

LOG2N = int(os.environ.get("LOG2N", "28"))
N = 1 << LOG2N
ROUNDS, WINDOW = 5, 20
GAIN = 0.5
MODES = (("FM", lib.POLAR_FM), ("PM", lib.POLAR_PM), ("AM", lib.POLAR_AM))


def torch_form(torch, mode, xc):
    """The composition on (S, n) complex64; FM's first column is the block's x[-1] = 0: 0."""
    if mode == lib.POLAR_FM:
        return torch.nn.functional.pad(torch.angle(xc[:, 1:] * xc[:, :-1].conj()) * GAIN, (1, 0))
    if mode == lib.POLAR_PM:
        return torch.angle(xc) * GAIN
    return torch.abs(xc) * GAIN


def main():
    import torch
    assert torch.cuda.is_available() and api.device_count() >= 1, "time_polar.py measures on the GPU"
    dev = torch.device("cuda:0")
    x = api.DeviceArray(2 * N)
    x.fill_synth(synth.SEED)
    y = api.DeviceArray(N)
    xt = torch.from_numpy(x.to_numpy()).to(dev)             # the same bytes, for torch
    yt = torch.empty(N, dtype=torch.float32, device=dev)
    xb = xt.view(torch.uint8)[:2 * N]
    timer = api.Timer()

    def lib_window(run, reps):
        timer.start()
        for _ in range(reps):
            run()
        timer.stop()
        return timer.elapsed_ms() / reps

    def torch_window(run, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            run()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    print(f"# 2^{LOG2N} samples per call; windows of {WINDOW} calls, median of {ROUNDS}; gain {GAIN}; torch {torch.__version__}")
    print(f"{'shape':>12s} {'mode':>4s} {'in':>5s} {'ms':>8s} {'frac':>6s} {'copy ms':>8s} {'of copy':>8s} {'torch ms':>9s} {'torch/blk':>9s} {'max diff':>9s}")
    for S in (1, 64):
        n = N // S
        check = min(n, (1 << 22) // S)
        for name, mode in MODES:
            for fmt in ("cf32", "u8"):
                h = api.Polar(mode, GAIN, n_streams=S)
                if fmt == "u8":
                    h.set_input_format(lib.FMT_U8)
                    src = xb.view(S, 2 * n)
                    conv = lambda s=src: torch.view_as_complex(((s.float() - 128.0) * (1.0 / 127.0)).view(S, -1, 2))
                    copy = lambda: yt.view(S, n).copy_(src[:, 0::2])
                else:
                    src = torch.view_as_complex(xt.view(S, n, 2))
                    conv = lambda s=src: s
                    copy = lambda: yt.view(S, n).copy_(torch.view_as_real(src)[:, :, 0])
                block = lambda: h.process_stream(x, n, y)     # (FM's carried sample moves on; the time does not depend on it)
                block()                                         # a fresh handle: the first column is 0 in FM
                api.sync()
                got = torch.from_numpy(np.stack([y.to_numpy(check, offset=s * n) for s in range(S)])).to(dev)
                xk = conv(src[:, :(2 if fmt == "u8" else 1) * check])
                ref = torch_form(torch, mode, xk)
                d = (got - ref).abs()
                if mode == lib.POLAR_AM:
                    diff = float(d.max() / ref.abs().max())
                else:
                    # +pi and -pi are one angle; the angle of an exact zero (a zero sample of the u8 stream) is anybody's: the
                    # block says +0, torch says the sign pattern of the zeros
                    arg = xk if mode == lib.POLAR_PM else torch.nn.functional.pad(xk[:, 1:] * xk[:, :-1].conj(), (1, 0))
                    d = torch.where(arg == 0, torch.zeros_like(d), torch.minimum(d, 2 * np.pi * GAIN - d))
                    diff = float(d.max() / GAIN)
                    del arg
                del got, ref, d, xk
                assert diff <= 1e-6, (S, name, fmt, diff)
                tform = lambda: torch_form(torch, mode, conv())
                lib_window(block, 3)
                torch_window(copy, 3)
                torch_window(tform, 2)
                t = {"block": [], "copy": [], "torch": []}
                for _ in range(ROUNDS):
                    t["block"].append(lib_window(block, WINDOW))
                    t["copy"].append(torch_window(copy, WINDOW))
                    t["torch"].append(torch_window(tform, max(2, WINDOW // 4)))
                ms, cms, tms = (float(np.median(t[k])) for k in ("block", "copy", "torch"))
                gb = (12 if fmt == "cf32" else 6) * N / 1e9
                print(f"{S:>3d} x 2^{n.bit_length() - 1:<4d} {name:>4s} {fmt:>5s} {ms:8.3f} {gb / ms / 6.29:6.3f} {cms:8.3f} {ms / cms:8.2f} {tms:9.3f} {tms / ms:9.2f} {diff:9.1e}",
                      flush=True)
                h.close()
                torch.cuda.empty_cache()
    x.free()
    y.free()


if __name__ == "__main__":
    main()
