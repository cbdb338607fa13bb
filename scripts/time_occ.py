#!/usr/bin/env python3
"""The spectrum occupancy detector (sfe_dsp_occ_*) over rows made by Psd on the device: unit-variance complex Gaussian
noise plus four on-bin tones of amplitude 0.5, a periodic Hann window, hop N, A = 16, scale 1 / (A sum w^2).  Psd makes
2^26 / (16 N) distinct rows from 2^26 samples; they are repeated on the device to fill a shape (a row's work does not
depend on its neighbours).  The detector runs at rank N/4, factor 8, gap 2, min_width 1, E = 16, shift 1, with and without
the mask.  `worst` replaces the rows by rows that are all occupied (every value 1, factor 0.5): one emission over every tile.
Beside every row:
  ceil   the bytes the call reads (4 N per row) at the measured copy ceiling of 6.29 TB/s; frac = ceil / ms;
  torch  the floor-plus-mask part of the law composed in torch on the same rows: kthvalue, a multiply, a clamp and a compare
         (no closing, no runs, no records: those need scans and a nonzero, which synchronises the host).  Its floor and
         threshold are held to the block's, bit for bit, on every row before anything is timed.
Times: device events around WINDOW consecutive calls behind a warm-up, the median of ROUNDS windows.
    python scripts/time_occ.py > profiles/occ/time_occ.txt
LOG2=20 shortens the large shapes to 2^20 bins per call."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api  # noqa: E402

LOG2 = int(os.environ.get("LOG2", "28"))
ROUNDS, WINDOW = 5, 10
A, E, FACTOR, GAP = 16, 16, 8.0, 2
SHAPES = ((4096, 1 << (LOG2 - 12)), (1024, 1 << (LOG2 - 10)), (256, 1 << (LOG2 - 8)), (4096, 64), (4096, 1))
PSD_SAMPLES = 1 << min(26, LOG2)
CEILING = 6.29e12


def main():
    import torch
    assert torch.cuda.is_available() and api.device_count() >= 1, "time_occ.py measures on the GPU"
    dev = torch.device("cuda:0")
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

    def psd_rows(N):
        """The distinct rows of one size, on the device: (PSD_SAMPLES / (A N), N) float32."""
        g = torch.Generator(device=dev).manual_seed(N)
        x = torch.randn(PSD_SAMPLES, 2, generator=g, device=dev) * float(np.sqrt(0.5))
        t = torch.arange(PSD_SAMPLES, device=dev) % N
        for b in (-507, -128, 3, 257):
            ph = (2.0 * np.pi * round(b * N / 1024) / N) * t
            x[:, 0] += 0.5 * torch.cos(ph)
            x[:, 1] += 0.5 * torch.sin(ph)
        w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)
        ps = api.Psd(w.astype(np.float32), N, A, scale=1.0 / (A * float(np.sum(w ** 2))))
        rows = torch.empty(PSD_SAMPLES // (A * N), N, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        assert ps.process_stream(x.data_ptr(), PSD_SAMPLES, rows.data_ptr()) == rows.shape[0]
        api.sync()
        ps.close()
        return rows

    print(f"# rows by Psd (A {A}, hop N, Hann) from noise plus four tones; rank N/4, factor {FACTOR}, gap {GAP}, E {E}, shift 1; "
          f"windows of {WINDOW} calls, median of {ROUNDS}; torch {torch.__version__}")
    print(f"{'N':>5s} {'rows':>8s} {'input':>6s} {'mask':>5s} {'ms':>9s} {'ceil ms':>8s} {'frac':>6s} {'torch ms':>9s} {'torch/blk':>9s} {'emissions/row':>13s}")
    made = {}
    for N, R in SHAPES:
        if N not in made:
            made[N] = psd_rows(N)
        d = made[N]
        rows = d.repeat(-(-R // d.shape[0]), 1)[:R].contiguous()
        info = torch.empty(R, 4, dtype=torch.int32, device=dev)
        rec = torch.empty(R, E, 8, dtype=torch.int32, device=dev)
        mask = torch.empty(R, N, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        for kind in ("psd", "worst"):
            if kind == "worst":
                rows.fill_(1.0)
                torch.cuda.synchronize()
            factor = FACTOR if kind == "psd" else 0.5
            h = api.Occ(N, N // 4, factor, 0.0, GAP, 1, E, True)

            def tform():
                floor = torch.kthvalue(rows, N // 4 + 1, dim=1).values
                thr = torch.clamp(floor * factor, min=0.0)
                return floor, thr, (rows > thr[:, None]).to(torch.uint8)

            tms = None
            for with_mask in (True, False):
                block = lambda: h.process_stream(rows.data_ptr(), R, info.data_ptr(), rec.data_ptr(), mask.data_ptr() if with_mask else None)
                assert block() == R
                api.sync()
                if with_mask:           # the torch form's floor and threshold are the block's, on every row
                    floor, thr, occ = tform()
                    got = info[:, :2].view(torch.float32)
                    assert torch.equal(got[:, 0].view(torch.int32), floor.view(torch.int32)), (N, R, kind)
                    assert torch.equal(got[:, 1].view(torch.int32), thr.view(torch.int32)), (N, R, kind)
                    assert bool((mask >= occ).all())            # the closing only adds bins (min_width is 1)
                    per_row = float(info[:, 2].float().mean())
                    del floor, thr, occ, got
                    torch_window(tform, 1)
                    tms = float(np.median([torch_window(tform, 2) for _ in range(ROUNDS)]))
                lib_window(block, 3)
                ms = float(np.median([lib_window(block, WINDOW) for _ in range(ROUNDS)]))
                ceil = 4.0 * N * R / CEILING * 1e3
                print(f"{N:>5d} {R:>8d} {kind:>6s} {'yes' if with_mask else 'no':>5s} {ms:9.4f} {ceil:8.4f} {ceil / ms:6.3f} {tms:9.3f} {tms / ms:9.2f} {per_row:13.2f}",
                      flush=True)
            h.close()
        del rows, info, rec, mask
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
