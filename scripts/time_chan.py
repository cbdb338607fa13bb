#!/usr/bin/env python3
"""The polyphase channelizer (sfe_dsp_chan_*) over 2^28 complex samples generated in HBM by sfe_dsp_synth_fill (u8: the
first 2^29 bytes of the same buffer as (I,Q) pairs), one call per launch, beside the same law composed in torch-ROCm in
the same process (strided view -> P tap-row sums -> torch.fft.ifft -> the D = M/2 sign) -- what a user would otherwise write.
HIP events, warm-up then 20 timed calls, mean.  bytes = algorithmic in + out: 8 B (cf32) or 2 B (u8) per input sample,
8 B per output sample (M n / D of them); frac = bytes / time / 8 TB/s.
    python scripts/time_chan.py > profiles/chan/time_chan.txt
SHAPES=256:256:16:cf32,... limits the run to those (M:D:P:fmt) shapes; TORCH=0 leaves the torch composition out."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api, lib, synth  # noqa: E402

REPS = 20
TORCH = os.environ.get("TORCH", "1") != "0"
n = 1 << int(os.environ.get("LOG2N", "28"))
SHAPES = [(M, D, P, fmt) for M in (16, 64, 256, 1024) for D in (M, M // 2) for P in (8, 16) for fmt in ("cf32", "u8")]
if os.environ.get("SHAPES"):
    want = {tuple(s.split(":")) for s in os.environ["SHAPES"].split(",")}
    SHAPES = [s for s in SHAPES if (str(s[0]), str(s[1]), str(s[2]), s[3]) in want]


def torch_channelize(xc, h, M, D):
    """(n,) complex64 cuda tensor -> (n // D, M) complex64: y[m, k] = sum_n h[n] x[mD - n] exp(-j 2 pi k (mD - n) / M)."""
    import torch
    L = h.numel()
    P = -(-L // M)
    hp = torch.zeros(P * M, device=xc.device)
    hp[:L] = h
    xp = torch.nn.functional.pad(torch.view_as_real(xc), (0, 0, P * M - 1, 0))     # P M - 1 zeros in front
    n_out = xc.numel() // D
    # frames[m, t] = x[mD - (PM - 1) + t]: row r of a frame holds x[mD - p - rM] at column M - 1 - p of row P - 1 - r
    acc = torch.zeros(n_out, M, 2, device=xc.device)
    for r in range(P):
        rows = xp.as_strided((n_out, M, 2), (2 * D, 2, 1), 2 * r * M)
        acc += rows * hp.flip(0)[r * M:(r + 1) * M].view(1, M, 1)
    v = torch.view_as_complex(acc).flip(1)                                         # v[m, p]
    y = torch.fft.ifft(v, dim=1) * M
    if D != M:
        k = torch.arange(M, device=xc.device)
        sign = 1.0 - 2.0 * ((k[None, :] * torch.arange(n_out, device=xc.device)[:, None]) & 1).float()
        y = y * sign
    return y


def main():
    import torch
    dev = torch.device("cuda:0")
    # the yardstick computes the same law: a small check against the library first
    m_chk, d_chk = 64, 32
    hc = synth.lowpass_taps(16 * m_chk - 3, 1.0 / m_chk)
    xs = synth.synth_cf32(1 << 14).view(np.complex64)
    ylib = api.Chan(hc, m_chk, d_chk).channelize(xs)[0]
    ytor = torch_channelize(torch.from_numpy(xs).to(dev), torch.from_numpy(hc).to(dev), m_chk, d_chk).T.contiguous().cpu().numpy()
    chk = synth.rel_rms(ytor.view(np.float32), ylib.view(np.float32))
    assert chk < 1e-5, chk

    x = api.DeviceArray(2 * n)
    x.fill_synth(synth.SEED)
    xt = torch.randn(n, dtype=torch.complex64, device=dev)
    bt = torch.randint(0, 256, (n, 2), dtype=torch.uint8, device=dev)
    t = api.Timer()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    print(f"# 2^{n.bit_length() - 1} complex samples per call; torch {torch.__version__}; torch composition checked against the "
          f"library at M={m_chk}, D={d_chk}: rel-RMS {chk:.1e}")
    print(f"{'M':>5s} {'D':>5s} {'P':>3s} {'in':>5s} {'ms':>8s} {'GB':>7s} {'frac':>6s} {'torch ms':>9s} {'x':>6s}")
    for M, D, P, fmt in SHAPES:
        h = synth.lowpass_taps(P * M, 1.0 / M)
        ch = api.Chan(h, M, D)
        if fmt == "u8":
            ch.set_input_format(lib.FMT_U8)
        n_out = n // D
        y = api.DeviceArray(2 * M * n_out)
        for _ in range(5):
            ch.process_stream(x, n, y)
        t.start()
        for _ in range(REPS):
            ch.process_stream(x, n, y)
        t.stop()
        ms = t.elapsed_ms() / REPS
        ch.close()
        y.free()
        gb = ((2 if fmt == "u8" else 8) * n + 8 * M * n_out) / 1e9
        if not TORCH:
            print(f"{M:5d} {D:5d} {P:3d} {fmt:>5s} {ms:8.3f} {gb:7.2f} {gb / ms / 8.0:6.3f}", flush=True)
            continue
        ht = torch.from_numpy(h).to(dev)

        def composed():
            src = torch.complex((bt[:, 0].float() - 128.0) * (1.0 / 127.0), (bt[:, 1].float() - 128.0) * (1.0 / 127.0)) \
                if fmt == "u8" else xt
            return torch_channelize(src, ht, M, D)
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
        print(f"{M:5d} {D:5d} {P:3d} {fmt:>5s} {ms:8.3f} {gb:7.2f} {gb / ms / 8.0:6.3f} {tms:9.3f} {tms / ms:6.1f}", flush=True)
    x.free()


if __name__ == "__main__":
    main()
