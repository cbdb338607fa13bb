#!/usr/bin/env python3
"""The streaming preamble correlator bank (sfe_dsp_corr_*) over 2^28 complex samples generated in HBM by sfe_dsp_synth_fill
(u8: the first 2^29 bytes of the same buffer as (I,Q) pairs; K = 16 on 2^26), one call per launch, B = V, peaks only (and
one dense row), beside the same law composed from what the library had before, in the same process: one complex-tap Fir
per template (taps conj(s_k) reversed; u8 through sfe_dsp_rx_u8_to_f32 first), then torch-ROCm for |c|^2, the window energy (a float64 cumsum differenced -- what a
user would write; the fused call sums the squares themselves), the division under the gate and the block maximum.  HIP
events, warm-up then 20 timed calls, mean (3 for the composition).  bytes = algorithmic in + out: 8 B (cf32) or 2 B (u8)
per input sample once, 8 B per template and block (+ 4 B per template and sample for the dense row); frac = bytes / time /
8 TB/s.
    python scripts/time_corr.py > profiles/corr/time_corr.txt
SHAPES=257:4:cf32:peaks,... limits the run to those (L:K:fmt:out) shapes; TORCH=0 leaves the composition out."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api, lib, synth  # noqa: E402

REPS = 20
GATE = 1e-6
TORCH = os.environ.get("TORCH", "1") != "0"
LOG2N = int(os.environ.get("LOG2N", "28"))
SHAPES = [(L, K, fmt, "peaks") for L in (13, 257, 1024, 2049) for K in (1, 4, 16) for fmt in ("cf32", "u8")] + [(257, 4, "cf32", "dense")]
if os.environ.get("SHAPES"):
    want = {tuple(s.split(":")) for s in os.environ["SHAPES"].split(",")}
    SHAPES = [s for s in SHAPES if (str(s[0]), str(s[1]), s[2], s[3]) in want]


def advance(L):
    return 4096 - 256 * -(-(L - 1) // 256)


def templates(L, K):
    t = np.stack([synth.synth_cf32(L, ch=100 + k).view(np.complex64) for k in range(K)])
    return (np.where(t.real >= 0, 1.0, -1.0) + 1j * np.where(t.imag >= 0, 1.0, -1.0)).astype(np.complex64)


class Composed:
    """The same law from a complex-tap Fir per template and torch; x is a float32 cuda tensor of 2n floats (cf32) whose
    first 2n bytes are the u8 stream."""

    def __init__(self, t, B, gate, fmt, n):
        import torch
        self.torch, self.B, self.gate, self.u8, self.n, self.L = torch, B, gate, fmt == "u8", n, t.shape[1]
        self.firs = [api.Fir(np.conj(tk)[::-1].copy(), data_complex=True) for tk in t]
        # a complex-tap Fir takes cf32 only: the bytes go through sfe_dsp_rx_u8_to_f32 first, one more pass
        self.xf = torch.empty(2 * n, dtype=torch.float32, device="cuda:0") if self.u8 else None
        self.E = [float(np.sum(np.abs(tk.astype(np.complex128)) ** 2)) for tk in t]
        self.c = torch.empty(n, dtype=torch.complex64, device="cuda:0")

    def __call__(self, x):
        torch, n, L = self.torch, self.n, self.L
        if self.u8:
            assert lib.load().sfe_dsp_rx_u8_to_f32(x.data_ptr(), self.xf.data_ptr(), 2 * n, None) == 0
            x = self.xf
        xr = x[:2 * n].view(n, 2)
        p = xr[:, 0] ** 2 + xr[:, 1] ** 2
        cs = torch.cumsum(p, 0, dtype=torch.float64)
        e = cs.clone()
        e[L:] -= cs[:-L]
        e = e.float()
        open_ = e > self.gate
        out = []
        for f, E in zip(self.firs, self.E):
            f.process_stream(x.data_ptr(), self.c.data_ptr(), n)
            cr = torch.view_as_real(self.c)
            m = torch.where(open_, (cr[:, 0] ** 2 + cr[:, 1] ** 2) / (E * e), 0.0)
            out.append((m,) + tuple(m.view(-1, self.B).max(dim=1)))
        return out

    def close(self):
        for f in self.firs:
            f.close()


def main():
    import torch
    dev = torch.device("cuda:0")
    L_ = lib.load()
    # the yardstick computes the same law: a small check against the library first
    Lc, Kc = 257, 2
    Bc = advance(Lc)
    nc = 4 * Bc
    tc = templates(Lc, Kc)
    xs = synth.synth_cf32(nc).view(np.complex64).copy()
    xs[5000:5000 + Lc] += 0.5 * tc[1]
    val, idx, dense = api.Corr(tc, Bc, GATE).search(xs, dense=True)
    comp = Composed(tc, Bc, GATE, "cf32", nc)
    got = comp(torch.from_numpy(xs.view(np.float32).copy()).to(dev))
    comp.close()
    chk = max(float(np.abs(got[k][0].cpu().numpy() - dense[0, k]).max()) for k in range(Kc))
    assert chk < 1e-5, chk
    assert all(np.array_equal(got[k][2].cpu().numpy(), idx[0, k]) for k in range(Kc))
    assert idx[0, 1, 1] == 5000 + Lc - 1 - Bc

    n_max = 1 << LOG2N
    x = torch.empty(2 * n_max, dtype=torch.float32, device=dev)
    assert L_.sfe_dsp_synth_fill(x.data_ptr(), 2 * n_max, synth.SEED, 0, 0, None) == 0
    torch.cuda.synchronize()
    t = api.Timer()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    print(f"# B = V, min_energy {GATE:g}; torch {torch.__version__}; composition (Fir per template + torch) checked against the "
          f"library at L={Lc}, K={Kc}: worst |dm| {chk:.1e}, same peak offsets")
    print(f"{'L':>5s} {'K':>3s} {'in':>5s} {'out':>6s} {'log2n':>5s} {'ms':>8s} {'GB':>7s} {'frac':>6s} {'Gsamp/s':>8s} {'comp ms':>9s} {'x':>6s}")
    for L, K, fmt, out in SHAPES:
        n = n_max >> 2 if K == 16 else n_max
        B = advance(L)
        n -= n % B
        tk = templates(L, K)
        cr = api.Corr(tk, B, GATE)
        if fmt == "u8":
            cr.set_input_format(lib.FMT_U8)
        nb = n // B
        d_val, d_idx = api.DeviceArray(K * nb), api.DeviceArray(K * nb)
        d_m = torch.empty(K * n, dtype=torch.float32, device=dev) if out == "dense" else None
        pm = d_m.data_ptr() if d_m is not None else None
        for _ in range(3):
            assert cr.process_stream(x.data_ptr(), n, d_val, d_idx, pm) == nb
        t.start()
        for _ in range(REPS):
            cr.process_stream(x.data_ptr(), n, d_val, d_idx, pm)
        t.stop()
        ms = t.elapsed_ms() / REPS
        cr.close()
        d_val.free()
        d_idx.free()
        del d_m
        gb = ((2 if fmt == "u8" else 8) * n + 8 * K * nb + (4 * K * n if out == "dense" else 0)) / 1e9
        line = f"{L:5d} {K:3d} {fmt:>5s} {out:>6s} {np.log2(n):5.2f} {ms:8.3f} {gb:7.2f} {gb / ms / 8.0:6.3f} {n / ms / 1e6:8.2f}"
        if not TORCH:
            print(line, flush=True)
            continue
        comp = Composed(tk, B, GATE, fmt, n)
        comp(x)
        torch.cuda.synchronize()
        reps_t = 3
        e0.record()
        for _ in range(reps_t):
            comp(x)
        e1.record()
        torch.cuda.synchronize()
        tms = e0.elapsed_time(e1) / reps_t
        comp.close()
        del comp
        torch.cuda.empty_cache()
        print(f"{line} {tms:9.3f} {tms / ms:6.1f}", flush=True)


if __name__ == "__main__":
    main()
