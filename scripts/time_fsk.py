#!/usr/bin/env python3
"""The 2-(G)FSK burst modem (sfe_dsp_fsk_*), both directions, at (sps, N, n_bursts) = (10, 280, 4096) -- short telemetry
bursts, BT 0.3 over four symbols -- and (4, 4120, 256) -- long frames, BT 0.5 over three: a 24-bit preamble, a one-symbol
boxcar as the matched filter, R = sps / 2, frames one sample apart in one stream.  mod in F32 and TX10; demod on the F32 stream
mod wrote, cf32, with and without the packed bits.  Beside every row:
  torch  the same law composed in torch on tensors that hold the same bytes.  mod: the bits unpacked to levels, zero-stuffed to
         the sample rate, conv1d with the pulse, cumsum, cos / sin.  demod: angle of x[n] conj(x[n-1]), conv1d with the
         matched filter, a gather of the symbol instants per timing candidate, the least-squares fit by its closed form, the
         soft values.  It is held to the block before anything is timed (mod: 2e-3 of amp -- a float32 cumsum over the frame;
         demod: the same timing and 2e-3 of scale).
  floor  the bytes a call must move over the 6.29 TB/s measured copy ceiling: mod stores 8 B a sample (F32) or 2.5 (TX10) and
         reads the payload; demod reads 8 B a sample once and stores 4 B a data bit (+ 1/8 with the packed bits).  What demod
         reads again for its filter chains comes through L2 and is not counted.
Times: device events around WINDOW consecutive calls behind a warm-up, the median of ROUNDS windows.
    python scripts/time_fsk.py > profiles/fsk/time_fsk.txt
BURSTS_DIV=16 shortens the calls.  Not measured here: u8 input, several streams, where the time goes by hardware counters."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api, lib, synth  # noqa: E402

ROUNDS, WINDOW = 5, 10
BURSTS_DIV = int(os.environ.get("BURSTS_DIV", "1"))
SHAPES = [(10, 0.3, 4, 280, 4096), (4, 0.5, 3, 4120, 256)]
PRE = [0, 1] * 8 + [0, 0, 1, 1, 0, 1, 0, 0]
CEILING = 6.29e12
H, AMP, SCALE = 0.5, 0.8, 2.0


def torch_mod(torch, by, pre_lev, g, sps, n_bits, F, out):
    """by (nb, bytes) uint8 -> out (nb, F) complex64."""
    shifts = torch.arange(7, -1, -1, device=by.device, dtype=torch.uint8)
    bits = ((by.unsqueeze(-1) >> shifts) & 1).reshape(by.shape[0], -1)[:, :n_bits]
    a = torch.cat([pre_lev.expand(by.shape[0], -1), 1.0 - 2.0 * bits.to(torch.float32)], dim=1)
    up = torch.zeros((a.shape[0], 1, a.shape[1] * sps), dtype=torch.float32, device=by.device)
    up[:, 0, ::sps] = a
    freq = torch.nn.functional.conv1d(up, g.flip(0).reshape(1, 1, -1), padding=g.numel() - 1)[:, 0, :F - 1]
    ph = torch.cumsum(freq, dim=1) * (np.pi * H)
    out[:, 0] = AMP
    out[:, 1:] = torch.complex(AMP * torch.cos(ph), AMP * torch.sin(ph))


def torch_demod(torch, x, step, nb, mf, e, sps, Lp, n_bits, delay, R, out):
    """x (n_in,) complex64 with burst b at b * step -> out (nb, n_bits) float32; returns tau (nb,)."""
    N = Lp + n_bits
    W = delay + R + (N - 1) * sps + mf.numel()
    w = x[:nb * step].reshape(nb, step)[:, :W]
    v = torch.angle(w[:, 1:] * w[:, :-1].conj())                 # v[i] of sample i + 1
    u = torch.nn.functional.conv1d(v.unsqueeze(1), mf.reshape(1, 1, -1))[:, 0]       # u[i] = sum m[j] v[i + j]: the law's u(i + 1)
    k = torch.arange(Lp, device=x.device) * sps
    taus = torch.arange(-R, R + 1, device=x.device)
    uk = u[:, (delay - 1 + taus[:, None] + k[None, :]).reshape(-1)].reshape(nb, 2 * R + 1, Lp)
    se, see = e.sum(), (e * e).sum()
    S1, Se = uk.sum(dim=-1), (uk * e).sum(dim=-1)
    num = Lp * Se - se * S1
    best = num.argmax(dim=1)
    rows = torch.arange(nb, device=x.device)
    dev = num[rows, best] / (Lp * see - se * se)
    dc = (S1[rows, best] - dev * se) / Lp
    kd = (Lp + torch.arange(n_bits, device=x.device)) * sps
    ud = torch.gather(u, 1, (delay - 1 + taus[best])[:, None] + kd[None, :])
    out[:] = SCALE * (ud - dc[:, None]) / dev[:, None]
    return taus[best]


def main():
    import torch
    assert torch.cuda.is_available() and api.device_count() >= 1, "time_fsk.py measures on the GPU"
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

    def measure(block, tform):
        lib_window(block, 3)
        torch_window(tform, 1)
        tb, tt = [], []
        for _ in range(ROUNDS):
            tb.append(lib_window(block, WINDOW))
            tt.append(torch_window(tform, 1))
        return float(np.median(tb)), float(np.median(tt))

    print(f"# windows of {WINDOW} calls, median of {ROUNDS}; bursts / {BURSTS_DIV}; torch {torch.__version__}; floor at {CEILING / 1e12:.2f} TB/s")
    print(f"{'sps':>4s} {'N':>5s} {'bursts':>6s} {'call':>12s} {'ms':>8s} {'GB':>7s} {'floor ms':>9s} {'frac':>6s} {'torch ms':>9s} {'torch/blk':>9s} {'diff':>8s}")
    rng = np.random.default_rng(synth.SEED)
    for sps, bt, span, N, nb in SHAPES:
        nb = max(2, nb // BURSTS_DIV)
        n_bits, Lp = N - len(PRE), len(PRE)
        g = synth.gfsk_pulse(bt, sps, span)
        mf = np.full(sps, 1.0 / sps, np.float32)
        delay, R = synth.fsk_delay(g.size, sps), sps // 2
        shape = (sps, g, H, PRE, n_bits, mf, delay, R, AMP, SCALE, 0.0)
        _, F, e, _ = api.fsk_plan(*shape)
        step, nbytes = F + 1, (n_bits + 7) // 8
        n_out = nb * step
        by = torch.from_numpy(rng.integers(0, 256, size=(nb, nbytes), dtype=np.uint8)).to(dev)
        x = torch.zeros(n_out, dtype=torch.complex64, device=dev)
        tx = torch.zeros(n_out // 2 * 5, dtype=torch.uint8, device=dev)
        y_t = torch.zeros((nb, F), dtype=torch.complex64, device=dev)
        soft, soft_t = (torch.zeros((nb, n_bits), dtype=torch.float32, device=dev) for _ in range(2))
        hard = torch.zeros((nb, nbytes), dtype=torch.uint8, device=dev)
        rec = torch.zeros((nb, 8), dtype=torch.float32, device=dev)
        st = torch.zeros(nb, dtype=torch.int32, device=dev)
        g_t, mf_t, e_t = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) for a in (g, mf, e))
        pre_lev = torch.from_numpy(1.0 - 2.0 * np.asarray(PRE, np.float32)).to(dev).reshape(1, -1)
        h = api.Fsk(*shape)
        ht = api.Fsk(*shape, out_fmt=lib.FMT_TX10)
        mod_f32 = lambda: h.mod(by.data_ptr(), nb, x.data_ptr(), n_out, 0, step)
        mod_tx10 = lambda: ht.mod(by.data_ptr(), nb, tx.data_ptr(), n_out, 0, step)
        t_mod = lambda: torch_mod(torch, by, pre_lev, g_t, sps, n_bits, F, y_t)
        dem = lambda: h.demod(x.data_ptr(), n_out, nb, soft.data_ptr(), None, None, None, rec.data_ptr(), st.data_ptr(), 0, step)
        dem_bits = lambda: h.demod(x.data_ptr(), n_out, nb, soft.data_ptr(), hard.data_ptr(), None, None, rec.data_ptr(), st.data_ptr(), 0, step)
        t_dem = lambda: torch_demod(torch, x, step, nb, mf_t, e_t, sps, Lp, n_bits, delay, R, soft_t)
        mod_f32()
        mod_tx10()
        t_mod()
        dem_bits()
        tau_t = t_dem()
        torch.cuda.synchronize()
        api.sync()
        k = min(nb, 8)
        d_mod = float((x.reshape(nb, step)[:k, :F] - y_t[:k]).abs().max() / AMP)
        assert d_mod <= 2e-3, (sps, N, "mod", d_mod)
        same_tau = rec[:k, 0] == tau_t[:k].to(torch.float32)       # (a tie between candidates may fall either way in torch's order of sums)
        assert int(st.abs().sum()) == 0 and int(same_tau.sum()) >= k // 2, (sps, N, "demod statuses / timing")
        d_dem = float((soft[:k] - soft_t[:k])[same_tau].abs().max() / SCALE)
        assert d_dem <= 2e-3, (sps, N, "demod", d_dem)
        assert bool((torch.from_numpy(np.unpackbits(hard[:k].cpu().numpy(), axis=1)[:, :n_bits]).to(dev) == (soft[:k] < 0)).all())
        rows = (("mod F32", mod_f32, t_mod, 8 * n_out + nb * nbytes, d_mod), ("mod TX10", mod_tx10, t_mod, n_out // 2 * 5 + nb * nbytes, d_mod),
                ("demod", dem, t_dem, 8 * n_out + nb * (4 * n_bits + 36), d_dem), ("demod +bits", dem_bits, t_dem, 8 * n_out + nb * (4 * n_bits + nbytes + 36), d_dem))
        for name, block, tform, moved, diff in rows:
            ms, tms = measure(block, tform)
            floor = moved / CEILING * 1e3
            print(f"{sps:>4d} {N:>5d} {nb:>6d} {name:>12s} {ms:8.3f} {moved / 1e9:7.3f} {floor:9.4f} {floor / ms:6.3f} {tms:9.3f} {tms / ms:9.2f} {diff:8.1e}",
                  flush=True)
        h.close()
        ht.close()
        del x, tx, y_t, soft, soft_t, hard, rec, st, by
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
