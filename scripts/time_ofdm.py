#!/usr/bin/env python3
"""One call of the OFDM burst receiver (sfe_dsp_ofdm_*): n_bursts bursts of T training and Ns data symbols, laid end to end
in HBM, into equalised data-bin symbols, channel estimates, records and statuses -- beside the same law composed in torch.
Every shape runs with cfo_mode 1 (cfo_skip = cp / 4), advance = cp / 4, an eighth of the used bins as pilots, zero-forcing
output, through a 3-tap channel with an offset of 0.13 subcarrier spacings; eight different bursts are repeated up to
n_bursts.  Both input formats are timed: cf32, and u8 (I,Q) byte pairs.
    ours   sfe_dsp_ofdm_process_stream: HIP events, 5 warm-up calls, then 5 windows of as many calls as take about 0.1 s
           (3 to 200): the median window's mean per call, with the fastest and the slowest window beside it.
    torch  the law as tensor operations on the same device buffer: the prefix products and their angle, the rotation (turn
           count in float64), torch.fft.fft over the gathered windows, and the per-bin arithmetic; u8 is converted first.
           Timed the same way.
    x      torch's time over ours.
    check  the rel-RMS of our symbols against torch's over the whole call, and the count of statuses that are not 0.
A single burst (the last row) is one workgroup working through its symbols one after another: a latency chain, not a
throughput figure.
    python scripts/time_ofdm.py > profiles/ofdm/time_ofdm.txt
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
# (N, cp, T, Ns, n_bursts)
ROWS = [(64, 16, 2, 6, 65536), (256, 32, 2, 14, 16384), (4096, 288, 1, 14, 1024), (4096, 288, 1, 14, 1)]
WANT = {(int(s.split(":")[0]), int(s.split(":")[1])) for s in os.environ["ROWS"].split(";")} if os.environ.get("ROWS") else None
TAPS = np.array([1.0, 0.0, 0.4 * np.exp(2.5j), 0.2 * np.exp(-0.8j)])
EPS = 0.13


def shape_of(N, cp, T, Ns):
    k = np.arange(N)
    f = np.where(k < N // 2, k, k - N)
    kind = np.where((np.abs(f) <= (N * 7) // 16) & (f != 0), 1, 0).astype(np.uint8)
    kind[(kind == 1) & (np.abs(f) % 8 == 4)] = 2
    train = synth.psk_symbols(N, 4, seed=synth.SEED + N).astype(np.complex64)
    pilot = synth.psk_symbols(N, 2, seed=synth.SEED + N + 1).astype(np.complex64)
    sign = np.where(synth.vit_bits(Ns, seed=synth.SEED + N + 2) == 1, -1, 1).astype(np.int8)
    return dict(n_fft=N, cp=cp, advance=cp // 4, n_train=T, n_data=Ns, kind=kind, train=train, pilot=pilot, pilot_sign=sign, cfo_mode=1,
                cfo_skip=cp // 4, out_mode=L.OFDM_OUT_ZF)


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
        kind = a["kind"]
        self.data = torch.from_numpy(np.flatnonzero(kind == 1)).to(dev)
        self.pil = torch.from_numpy(np.flatnonzero(kind == 2)).to(dev)
        self.used = torch.cat([self.data, self.pil])
        tr = a["train"].astype(np.complex128)[self.used.cpu().numpy()]
        self.c = torch.from_numpy((np.conj(tr) / (a["n_train"] * np.abs(tr) ** 2)).astype(np.complex64)).to(dev)
        want = a["pilot"][self.pil.cpu().numpy()][None, :] * a["pilot_sign"].astype(np.float32)[:, None]
        self.want = torch.from_numpy(want.astype(np.complex64)).to(dev)           # (Ns, Np)
        N, Lsym, nsym = a["n_fft"], a["n_fft"] + a["cp"], a["n_train"] + a["n_data"]
        self.n = torch.arange(nsym * Lsym, dtype=torch.float64, device=dev) / N

    def __call__(self, x):
        """x: (nb, (T + Ns)(N + cp)) complex64 -> symbols (nb, Ns, Nd)."""
        a = self.a
        N, cp, g, T, q = a["n_fft"], a["cp"], a["advance"], a["n_train"], a["cfo_skip"]
        nb = x.shape[0]
        r = x.view(nb, -1, N + cp)
        gamma = (r[:, :, q + N:cp + N] * r[:, :, q:cp].conj()).sum(dim=(1, 2))
        eps = torch.angle(gamma) / (2.0 * np.pi)
        turn = eps.double()[:, None] * self.n[None, :]
        turn = (turn - torch.round(turn)).float()
        r = (x * torch.polar(torch.ones_like(turn), -2.0 * np.pi * turn)).view(nb, -1, N + cp)
        Y = torch.fft.fft(r[:, :, cp - g:cp - g + N], dim=2)
        nd = self.data.numel()
        H = Y[:, :T, self.used].sum(dim=1) * self.c[None, :]
        Hd, Hp = H[:, :nd], H[:, nd:]
        P = (Y[:, T:, self.pil] * (Hp[:, None, :] * self.want[None, :, :]).conj()).sum(dim=2)
        phi = P / P.abs()
        return Y[:, T:, self.data] * (Hd[:, None, :] * phi[:, :, None]).conj() / (Hd.abs() ** 2)[:, None, :]


def main():
    dev = torch.device("cuda")
    print("# ms per call; cfo_mode 1, pilots on an eighth of the used bins, zero-forcing output; torch %s" % torch.__version__)
    print(f"{'N':>5s} {'cp':>4s} {'T':>2s} {'Ns':>3s} {'bursts':>6s} {'fmt':>4s} {'ms':>9s} {'min':>9s} {'max':>9s} {'reps':>4s} {'us/burst':>9s} "
          f"{'Msample/s':>10s} {'torch ms':>9s} {'x':>7s}   check")
    for N, cp, T, Ns, nb in ROWS:
        if WANT is not None and (N, nb) not in WANT:
            continue
        a = shape_of(N, cp, T, Ns)
        Nd = int(np.count_nonzero(a["kind"] == 1))
        reach = (T + Ns) * (N + cp)
        rng = np.random.default_rng(N + nb)
        nk = min(nb, KINDS)
        kinds = np.stack([synth.ofdm_signal(N, cp, T, a["kind"], a["train"], reach, 0, bits=rng.integers(0, 2, 2 * Ns * Nd).astype(np.uint8),
                                            pilot=a["pilot"], pilot_sign=a["pilot_sign"], taps=TAPS, eps=EPS) for _ in range(nk)])
        kinds = (kinds * (0.7 / np.abs(kinds.view(np.float32)).max())).astype(np.complex64)
        by = np.clip(np.rint(kinds.view(np.float32).astype(np.float64) * 127.0 + 128.0), 0, 255).astype(np.uint8)
        pick = torch.arange(nb, device=dev) % nk
        law = TorchLaw(a, dev)
        h = api.Ofdm(**a)
        out = torch.empty((nb, Ns, Nd), dtype=torch.complex64, device=dev)
        chan = torch.empty((nb, N), dtype=torch.complex64, device=dev)
        rec = torch.empty((nb, 8), dtype=torch.float32, device=dev)
        st = torch.empty(nb, dtype=torch.int32, device=dev)
        for fmt in ("cf32", "u8"):
            u8 = fmt == "u8"
            x = torch.from_numpy(by if u8 else kinds).to(dev)[pick].contiguous()
            torch.cuda.synchronize()
            h.set_input_format(L.FMT_U8 if u8 else L.FMT_F32)

            def ours():
                h.process_stream(x.data_ptr(), nb * reach, nb, out.data_ptr(), None, None, chan.data_ptr(), rec.data_ptr(), st.data_ptr(),
                                 start_step=reach)

            def theirs():
                xc = torch.view_as_complex(((x.float() - 128.0) * (1.0 / 127.0)).view(nb, reach, 2)) if u8 else x
                return law(xc)

            ms, lo, hi, reps = time_calls(ours)
            tms = time_calls(theirs)[0]
            want = theirs()
            torch.cuda.synchronize()
            err = float(torch.sqrt(((out - want).abs() ** 2).sum() / (want.abs() ** 2).sum()))
            bad = int((st != 0).sum())
            print(f"{N:5d} {cp:4d} {T:2d} {Ns:3d} {nb:6d} {fmt:>4s} {ms:9.4f} {lo:9.4f} {hi:9.4f} {reps:4d} {ms * 1e3 / nb:9.3f} "
                  f"{nb * reach / (ms * 1e-3) / 1e6:10.1f} {tms:9.4f} {tms / ms:7.2f}   rel-RMS against torch {err:.2e}; statuses not 0: {bad}",
                  flush=True)
            del x, want
        h.close()
        del out, chan, rec, st, law
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
