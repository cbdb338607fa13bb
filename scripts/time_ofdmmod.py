#!/usr/bin/env python3
"""One call of the OFDM burst modulator (sfe_dsp_ofdmmod_*): n_bursts rows of coded bytes in HBM become n_bursts frames of T
training and Ns data symbols laid end to end (start_step = F, no gaps) -- beside the same law composed in torch.  Every
shape is the receiver's of scripts/time_ofdm.py: an eighth of the used bins as pilots, BITS mode, order 4; amp is chosen so
that a sample's RMS is 0.15 (the wire format wraps at 1.0); eight different rows are repeated up to n_bursts.  Both output
formats are timed: cf32, and the 10-bit transmit wire format.
    ours   sfe_dsp_ofdmmod_process_stream: HIP events, 5 warm-up calls, then 5 windows of as many calls as take about 0.1 s
           (3 to 200): the median window's mean per call, with the fastest and the slowest window beside it.
    torch  the law as tensor operations on the same device buffers: the bytes unpacked to bits, the bits mapped and scattered
           to the bins beside the training and pilot tables, torch.fft.ifft, the prefix concatenated in front; for TX10 the
           quantiser and the packing of 5-byte groups behind it.  Timed the same way.
    GB/s   bytes stored per second (8 per sample in cf32, 2.5 under TX10), and that as a share of the 6.29 TB/s copy ceiling.
    x      torch's time over ours.
    check  cf32: the rel-RMS of our stream against torch's over the whole call.  TX10: the 10-bit words that differ from
           torch's by one step (a float32 value on either side of a step) and by more.
The last row is one burst: its 15 symbols are 15 workgroups, where the receiver's one workgroup per burst takes 0.20 ms.
    python scripts/time_ofdmmod.py > profiles/ofdmmod/time_ofdmmod.txt
ROWS="n_fft:n_bursts;..." limits the run to those rows."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simplefe_amd import api, synth  # noqa: E402
from simplefe_amd import lib as L  # noqa: E402

WARM, WINDOWS, KINDS = 5, 5, 8
COPY_CEILING = 6.29e12
# (N, cp, T, Ns, n_bursts)
ROWS = [(64, 16, 2, 6, 65536), (256, 32, 2, 14, 16384), (4096, 288, 1, 14, 1024), (4096, 288, 1, 14, 1)]
WANT = {(int(s.split(":")[0]), int(s.split(":")[1])) for s in os.environ["ROWS"].split(";")} if os.environ.get("ROWS") else None


def shape_of(N, cp, T, Ns, out_fmt):
    k = np.arange(N)
    f = np.where(k < N // 2, k, k - N)
    kind = np.where((np.abs(f) <= (N * 7) // 16) & (f != 0), 1, 0).astype(np.uint8)
    kind[(kind == 1) & (np.abs(f) % 8 == 4)] = 2
    train = synth.psk_symbols(N, 4, seed=synth.SEED + N).astype(np.complex64)
    pilot = synth.psk_symbols(N, 2, seed=synth.SEED + N + 1).astype(np.complex64)
    sign = np.where(synth.vit_bits(Ns, seed=synth.SEED + N + 2) == 1, -1, 1).astype(np.int8)
    amp = float(np.float32(0.15 * N / np.sqrt(np.count_nonzero(kind))))
    return dict(n_fft=N, cp=cp, n_train=T, n_data=Ns, kind=kind, train=train, pilot=pilot, pilot_sign=sign, amp=amp, order=4,
                in_mode=L.OFDMMOD_IN_BITS, out_fmt=out_fmt)


def time_calls(run):
    """(median, fastest, slowest) window's mean ms per call, calls per window."""
    t = api.Timer()
    for _ in range(WARM):
        run()
    t.start()
    run()
    t.stop()
    reps = int(min(200, max(3, np.ceil(100.0 / max(t.elapsed_ms(), 1e-3)))))
    ms = []
    for _ in range(WINDOWS):
        t.start()
        for _ in range(reps):
            run()
        t.stop()
        ms.append(t.elapsed_ms() / reps)
    return float(np.median(ms)), min(ms), max(ms), reps


class TorchLaw:
    """The law of include/sfe_dsp.h as tensor operations; the tables live on the device."""

    def __init__(self, a, dev):
        self.a = a
        kind, amp = a["kind"], np.float32(a["amp"])
        self.data = torch.from_numpy(np.flatnonzero(kind == 1)).to(dev)
        self.pil = torch.from_numpy(np.flatnonzero(kind == 2)).to(dev)
        ta = np.where(kind != 0, a["train"] * amp, 0).astype(np.complex64)
        pa = (a["pilot"][kind == 2][None, :] * amp * a["pilot_sign"].astype(np.float32)[:, None]).astype(np.complex64)
        self.ta, self.pa = torch.from_numpy(ta).to(dev), torch.from_numpy(pa).to(dev)          # (N,), (Ns, Np)
        self.a4 = float(np.float32(np.float64(amp) / np.sqrt(2.0)))
        self.shifts = torch.arange(7, -1, -1, dtype=torch.uint8, device=dev)

    def __call__(self, by, tx10):
        """by: (nb, ceil(2 Ns Nd / 8)) uint8 -> the stream, (nb F,) complex64 or (nb F / 2 * 5,) uint8."""
        a = self.a
        N, cp, T, Ns = a["n_fft"], a["cp"], a["n_train"], a["n_data"]
        nb, nd = by.shape[0], self.data.numel()
        bits = ((by[:, :, None] >> self.shifts[None, None, :]) & 1).view(nb, -1)[:, :2 * Ns * nd].view(nb, Ns, nd, 2)
        s = torch.view_as_complex((self.a4 * (1.0 - 2.0 * bits.float())).contiguous())
        X = torch.zeros((nb, T + Ns, N), dtype=torch.complex64, device=by.device)
        X[:, :T, :] = self.ta[None, None, :]
        X[:, T:, self.data] = s
        X[:, T:, self.pil] = self.pa[None, :, :]
        x = torch.fft.ifft(X, dim=2)
        y = torch.cat([x[:, :, N - cp:], x], dim=2).reshape(-1)
        if not tx10:
            return y
        u = (((torch.view_as_real(y) * 511.0).int() << 16 >> 16) + 512) & 0x3FF
        u = u.view(-1, 4)
        g = torch.empty((u.shape[0], 5), dtype=torch.uint8, device=by.device)
        g[:, 0] = ((u[:, 0] >> 8) | ((u[:, 1] >> 8) << 2) | ((u[:, 2] >> 8) << 4) | ((u[:, 3] >> 8) << 6)).to(torch.uint8)
        g[:, 1:] = (u & 0xFF).to(torch.uint8)
        return g.view(-1)


def words10(b):
    """(groups, 4) int32 10-bit words of wire-format bytes."""
    b = b.view(-1, 5).int()
    return torch.stack([((b[:, 0] >> (2 * i)) & 3) << 8 | b[:, 1 + i] for i in range(4)], dim=1)


def main():
    dev = torch.device("cuda")
    print("# ms per call; frames end to end, BITS mode, order 4, pilots on an eighth of the used bins; torch %s" % torch.__version__)
    print(f"{'N':>5s} {'cp':>4s} {'T':>2s} {'Ns':>3s} {'bursts':>6s} {'fmt':>4s} {'ms':>9s} {'min':>9s} {'max':>9s} {'reps':>4s} {'us/burst':>9s} "
          f"{'Msample/s':>10s} {'GB/s':>8s} {'of copy':>7s} {'torch ms':>9s} {'x':>7s}   check")
    for N, cp, T, Ns, nb in ROWS:
        if WANT is not None and (N, nb) not in WANT:
            continue
        for fmt in ("cf32", "tx10"):
            tx10 = fmt == "tx10"
            a = shape_of(N, cp, T, Ns, L.FMT_TX10 if tx10 else L.FMT_F32)
            h = api.OfdmMod(**a)
            F, nbytes = h.frame_len, h.n_bytes
            rng = np.random.default_rng(N + nb)
            nk = min(nb, KINDS)
            kinds = rng.integers(0, 256, size=(nk, nbytes), dtype=np.uint8)
            by = torch.from_numpy(kinds).to(dev)[torch.arange(nb, device=dev) % nk].contiguous()
            n_out = nb * F
            out_bytes = n_out // 2 * 5 if tx10 else 8 * n_out
            out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
            law = TorchLaw(a, dev)
            torch.cuda.synchronize()

            def ours():
                h.process_stream(by.data_ptr(), nb, out.data_ptr(), n_out, 0, F)

            def theirs():
                return law(by, tx10)

            ms, lo, hi, reps = time_calls(ours)
            tms = time_calls(theirs)[0]
            want = theirs()
            torch.cuda.synchronize()
            if tx10:
                d = (words10(out) - words10(want)).abs()
                check = "10-bit words off by one step against torch %d of %d; by more: %d" % (int((d == 1).sum()), d.numel(), int((d > 1).sum()))
            else:
                got = out.view(torch.float32).view(-1, 2)
                got = torch.view_as_complex(got)
                err = float(torch.sqrt(((got - want).abs() ** 2).sum() / (want.abs() ** 2).sum()))
                check = "rel-RMS against torch %.2e" % err
            rate = out_bytes / (ms * 1e-3)
            print(f"{N:5d} {cp:4d} {T:2d} {Ns:3d} {nb:6d} {fmt:>4s} {ms:9.4f} {lo:9.4f} {hi:9.4f} {reps:4d} {ms * 1e3 / nb:9.3f} "
                  f"{n_out / (ms * 1e-3) / 1e6:10.1f} {rate / 1e9:8.1f} {100.0 * rate / COPY_CEILING:6.1f}% {tms:9.4f} {tms / ms:7.2f}   {check}",
                  flush=True)
            h.close()
            del by, out, want, law
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
