#!/usr/bin/env python3
"""The polyphase synthesis filter bank (sfe_dsp_combine_*) writing 2^28 complex output samples per call from channel
inputs generated in HBM by sfe_dsp_synth_fill, one call per launch, beside the same law composed in torch-ROCm in the
same process (torch.fft.ifft over the channels -> the D = M/2 rotation -> J tap-row sums into the output phases) --
what a user would otherwise write.  HIP events, warm-up then 20 timed calls, mean.  bytes = algorithmic in + out:
8 B per input sample (M n / D of them), 8 B (F32) or 2.5 B (TX10) per output sample; frac = bytes / time / 8 TB/s.
The shapes are time_chan.py's mirrors: the same (M, D, P) with P = L / M taps per channel, F32 or TX10 output.
    python scripts/time_combine.py > profiles/combine/time_combine.txt
SHAPES=256:256:16:f32,... limits the run to those (M:D:P:fmt) shapes; TORCH=0 leaves the torch composition out."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api, lib, synth  # noqa: E402

REPS = 20
TORCH = os.environ.get("TORCH", "1") != "0"
n = 1 << int(os.environ.get("LOG2N", "28"))
SHAPES = [(M, D, P, fmt) for M in (16, 64, 256, 1024) for D in (M, M // 2) for P in (8, 16) for fmt in ("f32", "tx10")]
if os.environ.get("SHAPES"):
    want = {tuple(s.split(":")) for s in os.environ["SHAPES"].split(",")}
    SHAPES = [s for s in SHAPES if (str(s[0]), str(s[1]), str(s[2]), s[3]) in want]


def torch_combine(X, g, M, D):
    """(M, n) complex64 cuda tensor -> (n D,) complex64: z[i] = sum_m g[i - mD] sum_k X_k[m] exp(+j 2 pi k i / M)."""
    import torch
    nn = X.shape[1]
    L = g.numel()
    Pd = -(-L // D)
    gp = torch.zeros(Pd * D, device=X.device)
    gp[:L] = g
    v = torch.fft.ifft(X, dim=0) * M                                    # v[q, m]
    v = v.T.contiguous()                                                # [m, q]
    if D != M:                                                          # row m rotated by m D mod M: u_m[c] = v_{c + mD}
        odd = torch.arange(nn, device=X.device) % 2 == 1
        v[odd] = torch.roll(v[odd], -M // 2, dims=1)
    vr = torch.view_as_real(v)                                          # [m, M, 2]
    vp = torch.nn.functional.pad(vr, (0, 0, 0, 0, Pd - 1, 0))          # Pd - 1 zero rows in front
    z = torch.zeros(nn, D, 2, device=X.device)
    gr = gp.view(Pd, D)
    for j in range(Pd):
        rows = vp[Pd - 1 - j:Pd - 1 - j + nn]                           # u_{m - j}
        col = (j * D) % M                                               # column (j D + r) mod M, r < D
        z += rows[:, col:col + D] * gr[j].view(1, D, 1)
    return torch.view_as_complex(z.reshape(nn * D, 2))


def main():
    import torch
    dev = torch.device("cuda:0")
    # the yardstick computes the same law: a small check against the library first
    m_chk, d_chk = 64, 32
    gc = synth.lowpass_taps(16 * m_chk - 3, 1.0 / m_chk)
    xs = np.stack([synth.synth_cf32(256, ch=k).view(np.complex64) for k in range(m_chk)])
    zlib = api.Combiner(gc, m_chk, d_chk).combine(xs)[0]
    ztor = torch_combine(torch.from_numpy(xs).to(dev), torch.from_numpy(gc).to(dev), m_chk, d_chk).cpu().numpy()
    chk = synth.rel_rms(ztor.view(np.float32), zlib.view(np.float32))
    assert chk < 1e-5, chk

    t = api.Timer()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    print(f"# 2^{n.bit_length() - 1} complex output samples per call; torch {torch.__version__}; torch composition checked "
          f"against the library at M={m_chk}, D={d_chk}: rel-RMS {chk:.1e}")
    print(f"{'M':>5s} {'D':>5s} {'P':>3s} {'out':>5s} {'ms':>8s} {'GB':>7s} {'frac':>6s} {'torch ms':>9s} {'x':>6s}")
    for M, D, P, fmt in SHAPES:
        g = synth.lowpass_taps(P * M, 1.0 / M)
        cb = api.Combiner(g, M, D)
        if fmt == "tx10":
            cb.set_output_format(lib.FMT_TX10)
        n_in = n // D
        x = api.DeviceArray(2 * M * n_in)
        x.fill_synth(synth.SEED)
        y = api.DeviceArray(2 * n)
        for _ in range(5):
            cb.process_stream(x, n_in, y)
        t.start()
        for _ in range(REPS):
            cb.process_stream(x, n_in, y)
        t.stop()
        ms = t.elapsed_ms() / REPS
        cb.close()
        x.free()
        y.free()
        gb = (8 * M * n_in + (2.5 if fmt == "tx10" else 8) * n) / 1e9
        if not TORCH:
            print(f"{M:5d} {D:5d} {P:3d} {fmt:>5s} {ms:8.3f} {gb:7.2f} {gb / ms / 8.0:6.3f}", flush=True)
            continue
        if fmt == "tx10":          # torch has no fused wire format: the F32 composition's time is the yardstick for both
            print(f"{M:5d} {D:5d} {P:3d} {fmt:>5s} {ms:8.3f} {gb:7.2f} {gb / ms / 8.0:6.3f} {tms:9.3f} {tms / ms:6.1f}", flush=True)
            continue
        gt = torch.from_numpy(g).to(dev)
        Xt = torch.randn(M, n_in, dtype=torch.complex64, device=dev)
        for _ in range(2):
            torch_combine(Xt, gt, M, D)
        torch.cuda.synchronize()
        reps_t = 3
        e0.record()
        for _ in range(reps_t):
            torch_combine(Xt, gt, M, D)
        e1.record()
        torch.cuda.synchronize()
        tms = e0.elapsed_time(e1) / reps_t
        del Xt
        torch.cuda.empty_cache()
        print(f"{M:5d} {D:5d} {P:3d} {fmt:>5s} {ms:8.3f} {gb:7.2f} {gb / ms / 8.0:6.3f} {tms:9.3f} {tms / ms:6.1f}", flush=True)


if __name__ == "__main__":
    main()
