#!/usr/bin/env python3
"""The streaming Welch spectrum estimator (sfe_dsp_psd_*) over 2^28 complex samples generated in HBM by sfe_dsp_synth_fill
(u8: the first 2^29 bytes of the same buffer as (I,Q) pairs), one call per launch, beside the same law composed in
torch-ROCm in the same process (as_strided frames -> window -> torch.fft.fft -> squared magnitude -> sum over A) -- what a
user would otherwise write.  HIP events, warm-up then 20 timed calls, mean (A divides the call's segments: every call is whole rows).
bytes = algorithmic in + out: 8 B (cf32) or 2 B (u8) per input sample once, 4 B per output bin; frac = bytes / time / 8 TB/s.
A = "all" is one row over every segment of the call.
    python scripts/time_psd.py > profiles/psd/time_psd.txt
SHAPES=1024:512:64:cf32,... limits the run to those (N:H:A:fmt) shapes; TORCH=0 leaves the torch composition out."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api, lib, synth  # noqa: E402

REPS = 20
TORCH = os.environ.get("TORCH", "1") != "0"
n = 1 << int(os.environ.get("LOG2N", "28"))
SHAPES = [(N, H, A, fmt) for N in (256, 1024, 4096) for H in (N, N // 2) for A in (1, 64, "all") for fmt in ("cf32", "u8")]
if os.environ.get("SHAPES"):
    want = {tuple(s.split(":")) for s in os.environ["SHAPES"].split(",")}
    SHAPES = [s for s in SHAPES if (str(s[0]), str(s[1]), str(s[2]), s[3]) in want]


def torch_psd(xc, w, H, A, scale):
    """(n,) complex64 cuda tensor -> (rows, N) float32: row r = scale sum over segments [rA, (r+1)A) of |fft(w x[seg])|^2,
    segment m being the N samples that end at (m + 1) H, zeros before the stream."""
    import torch
    N = w.numel()
    q = xc.numel() // H
    xp = torch.nn.functional.pad(torch.view_as_real(xc), (0, 0, N - H, 0))         # N - H zeros in front
    frames = torch.view_as_complex(xp.as_strided((q, N, 2), (2 * H, 2, 1)))
    X = torch.fft.fft(frames * w[None, :], dim=1)
    P = X.real * X.real + X.imag * X.imag
    rows = q // A
    return P[:rows * A].view(rows, A, N).sum(dim=1) * scale


def main():
    import torch
    dev = torch.device("cuda:0")
    # the yardstick computes the same law: a small check against the library first
    n_chk, h_chk, a_chk = 1024, 384, 5
    wc = np.hanning(n_chk).astype(np.float32)
    xs = synth.synth_cf32(h_chk * a_chk * 6).view(np.complex64)
    ylib = api.Psd(wc, h_chk, a_chk, scale=0.25).spectrum(xs)[0]
    ytor = torch_psd(torch.from_numpy(xs).to(dev), torch.from_numpy(wc).to(dev), h_chk, a_chk, 0.25).cpu().numpy()
    chk = synth.rel_rms(ytor, ylib)
    assert ytor.shape == ylib.shape and chk < 1e-5, chk

    x = api.DeviceArray(2 * n)
    x.fill_synth(synth.SEED)
    xt = torch.randn(n, dtype=torch.complex64, device=dev)
    bt = torch.randint(0, 256, (n, 2), dtype=torch.uint8, device=dev)
    t = api.Timer()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    print(f"# 2^{n.bit_length() - 1} complex samples per call; torch {torch.__version__}; torch composition checked against the "
          f"library at N={n_chk}, H={h_chk}, A={a_chk}: rel-RMS {chk:.1e}")
    print(f"{'N':>5s} {'H':>5s} {'A':>8s} {'in':>5s} {'ms':>8s} {'GB':>7s} {'frac':>6s} {'torch ms':>9s} {'x':>6s}")
    for N, H, A, fmt in SHAPES:
        q = n // H
        a = q if A == "all" else A
        w = np.hanning(N).astype(np.float32)
        scale = 1.0 / (a * float(np.sum(w.astype(np.float64) ** 2)))
        ps = api.Psd(w, H, a, scale=scale)
        if fmt == "u8":
            ps.set_input_format(lib.FMT_U8)
        rows = q // a
        y = api.DeviceArray(rows * N)
        assert q % a == 0                   # every call is whole rows: back-to-back calls need no reset
        for _ in range(5):
            assert ps.process_stream(x, n, y) == rows
        t.start()
        for _ in range(REPS):
            ps.process_stream(x, n, y)
        t.stop()
        ms = t.elapsed_ms() / REPS
        ps.close()
        y.free()
        gb = ((2 if fmt == "u8" else 8) * n + 4 * N * rows) / 1e9
        if not TORCH:
            print(f"{N:5d} {H:5d} {str(A):>8s} {fmt:>5s} {ms:8.3f} {gb:7.2f} {gb / ms / 8.0:6.3f}", flush=True)
            continue
        wt = torch.from_numpy(w).to(dev)

        def composed():
            src = torch.complex((bt[:, 0].float() - 128.0) * (1.0 / 127.0), (bt[:, 1].float() - 128.0) * (1.0 / 127.0)) \
                if fmt == "u8" else xt
            return torch_psd(src, wt, H, a, scale)
        for _ in range(2):
            composed()
        torch.cuda.synchronize()
        reps_t = 3
        e0.record()
        for _ in range(reps_t):
            composed()
        e1.record()
        torch.cuda.synchronize()
        tms = e0.elapsed_time(e1) / reps_t
        torch.cuda.empty_cache()
        print(f"{N:5d} {H:5d} {str(A):>8s} {fmt:>5s} {ms:8.3f} {gb:7.2f} {gb / ms / 8.0:6.3f} {tms:9.3f} {tms / ms:6.1f}", flush=True)
    x.free()


if __name__ == "__main__":
    main()
