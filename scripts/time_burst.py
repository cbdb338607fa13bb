#!/usr/bin/env python3
"""One call of the burst demodulator (sfe_dsp_burst_*): n_bursts windows of a cf32 stream in HBM, one every (N + 2) sps
samples, into N symbols each, with records and statuses; Lp = 32, lag = 4, timing estimated:
    ours   sfe_dsp_burst_process_stream: HIP events, 20 warm-up calls, then 5 windows of 1000 calls each (8 to 80 ms a
           window): the median window's mean per call, with the fastest and the slowest window beside it.  Nothing
           synchronises inside a window.  The input is the same buffer in every call: the batched rows' 34 to 105 MB may stay
           in the last-level cache from one call to the next, so these are times on a resident input.
Beside each row, in the same process, the two compositions it replaces:
    torch  the same law composed of torch-ROCm tensor operations over the same device buffer (float32, the turn count in
           float64; the gate, the range and the finite check are left out, in torch's favour); HIP events, 5 warm-up calls,
           then 3 windows of 20 calls, median and range as above.  Its f of burst 0 is compared with the block's.
    host   the round trip: copy the windows down, sfe_dsp_burst_plan (float64 on one host core), copy the symbols up;
           wall clock, one warm-up then 3 calls, median and range.
The check column compares the records of the first four bursts with the plan's.
    python scripts/time_burst.py > profiles/burst/time_burst.txt
TORCH=0 leaves the torch composition out; SHAPES="sps:N:n_bursts;..." limits the run to those rows."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api, synth  # noqa: E402

WARM, WINDOWS, REPS, TORCH_WARM, TORCH_WINDOWS, TORCH_REPS, HOST_REPS, CHECK = 20, 5, 1000, 5, 3, 20, 3, 4
TORCH = os.environ.get("TORCH", "1") != "0"
SHAPES = [(10, 256, 1), (10, 256, 4096), (4, 4096, 256), (50, 1024, 256)]
WANT = {tuple(int(v) for v in s.split(":")) for s in os.environ["SHAPES"].split(";")} if os.environ.get("SHAPES") else None
LP, LAG = 32, 4


def time_calls(run, warm, windows, reps):
    """(median, fastest, slowest) window's mean ms per call."""
    t = api.Timer()
    for _ in range(warm):
        run()
    ms = []
    for _ in range(windows):
        t.start()
        for _ in range(reps):
            run()
        t.stop()
        ms.append(t.elapsed_ms() / reps)
    return float(np.median(ms)), min(ms), max(ms)


class _Cai:
    """A window of a DeviceArray for torch.as_tensor (the CUDA array interface, which torch-ROCm reads too)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def torch_law(torch, X, pre, sps, N, lag):
    """The law on a (n_bursts, (N + 2) sps) complex64 tensor of reaches: (symbols, f)."""
    nb, Lp, dev = X.shape[0], pre.shape[0], X.device
    w = torch.exp(-2j * torch.pi * torch.arange(sps, device=dev) / sps).to(torch.complex64)
    p = (X[:, sps:(N + 1) * sps].abs() ** 2).reshape(nb, N, sps).sum(1).to(torch.complex64)
    c = (p * w).sum(1)
    tau = -sps * torch.angle(c) / (2 * torch.pi)
    tau = torch.where(tau <= -0.5 * sps, tau + sps, tau)
    m = torch.floor(tau)
    mu = (tau - m)[:, None]
    at = sps + torch.arange(N, device=dev)[None, :] * sps + m.long()[:, None] - 1
    L4 = (-mu * (mu - 1) * (mu - 2) / 6, (mu + 1) * (mu - 1) * (mu - 2) / 2, -(mu + 1) * mu * (mu - 2) / 2, (mu + 1) * mu * (mu - 1) / 6)
    y = sum(L4[q] * torch.gather(X, 1, at + q) for q in range(4))
    z = y[:, :Lp] * pre.conj()
    f = torch.angle((z[:, lag:] * z[:, :-lag].conj()).sum(1)) / (2 * torch.pi * lag)
    k = torch.arange(N, device=dev, dtype=torch.float64)[None, :]

    def unturn(t):
        t = (t - torch.round(t)).to(torch.float32)
        return torch.polar(torch.ones_like(t), -2 * torch.pi * t)

    S = (z * unturn(f.double()[:, None] * k[:, :Lp])).sum(1)
    theta, a = torch.angle(S) / (2 * torch.pi), S.abs() / (pre.abs() ** 2).sum()
    return y * unturn(theta.double()[:, None] + f.double()[:, None] * k) / a[:, None], f


def main():
    torch = None
    if TORCH:
        import torch
        print(f"# torch {torch.__version__}")
    print("# Lp = %d, lag = %d, one burst every (N + 2) sps samples; ms per call" % (LP, LAG))
    print(f"{'sps':>3s} {'N':>5s} {'bursts':>6s} {'ms':>9s} {'min':>7s} {'max':>7s} {'torch ms':>9s} {'min':>6s} {'max':>6s} {'x':>7s} {'host ms':>9s} "
          f"{'min':>8s} {'max':>8s} {'x':>8s}   check")
    lib = api._l.load()
    for sps, N, nb in SHAPES:
        if WANT is not None and (sps, N, nb) not in WANT:
            continue
        reach = (N + 2) * sps
        a = synth.psk_symbols(N, 4, seed=synth.SEED + N)
        one = synth.burst_signal(a, sps, reach, sps, 0.3, 0.01, 0.7, 0.5)
        x = np.tile(one, nb)
        pre = a[:LP].astype(np.complex64)
        d_x, d_out = api.DeviceArray.from_numpy(x.view(np.float32)), api.DeviceArray(nb * N * 2)
        d_rec, d_st = api.DeviceArray(nb * 8), api.DeviceArray(nb)
        h = api.Burst(pre, sps, N, LAG)
        ms, lo, hi = time_calls(lambda: h.process_stream(d_x, x.size, nb, d_out, None, None, d_rec, d_st, sps, reach), WARM, WINDOWS, REPS)
        api.sync()
        rec, st = d_rec.to_numpy().reshape(nb, 8), d_st.to_numpy().view(np.int32)
        k = min(nb, CHECK)
        prec = api.burst_plan(pre, sps, N, LAG, x=x[:k * reach], n_bursts=k, start_base=sps, start_step=reach)[1]
        chk = f"status {int(st.max())}, max |record - plan| {np.abs(rec[:k, :6] - prec[:, :6]).max():.1e}"
        h.close()

        tnote = f"{'':>9s} {'':>6s} {'':>6s} {'':>7s}"
        if torch is not None:
            try:
                dev = torch.device("cuda:0")
                X = torch.view_as_complex(torch.as_tensor(_Cai(d_x.ptr, (nb, reach, 2), "<f4"), device=dev))
                tp = torch.as_tensor(pre, device=dev)
                last = []

                def run():
                    last[:] = [torch_law(torch, X, tp, sps, N, LAG)]
                tm, tlo, thi = time_calls(run, TORCH_WARM, TORCH_WINDOWS, TORCH_REPS)
                torch.cuda.synchronize()
                tnote = f"{tm:9.3f} {tlo:6.3f} {thi:6.3f} {tm / ms:7.2f}"
                chk += f"; |f - torch's| of burst 0 {abs(float(last[0][1][0]) - rec[0, 1]):.1e}"
                del X, last
                torch.cuda.empty_cache()
            except Exception as e:
                tnote = f"{'n/a':>9s} {'':>6s} {'':>6s} {'':>7s}"
                chk += f"; torch: {type(e).__name__}: {str(e)[:60]}"

        host = np.empty_like(x)

        def round_trip():
            api.check(lib.sfe_dsp_memcpy_d2h(host.ctypes.data, d_x.ptr, host.nbytes, None))
            api.sync()
            sym = api.burst_plan(pre, sps, N, LAG, x=host, n_bursts=nb, start_base=sps, start_step=reach)[0]
            api.check(lib.sfe_dsp_memcpy_h2d(d_out.ptr, sym.ctypes.data, sym.nbytes, None))
            api.sync()
        round_trip()
        ths = []
        for _ in range(HOST_REPS):
            t0 = time.perf_counter()
            round_trip()
            ths.append((time.perf_counter() - t0) * 1e3)
        th = float(np.median(ths))
        print(f"{sps:3d} {N:5d} {nb:6d} {ms:9.4f} {lo:7.4f} {hi:7.4f} {tnote} {th:9.3f} {min(ths):8.3f} {max(ths):8.3f} {th / ms:8.1f}   {chk}", flush=True)
        for d in (d_x, d_out, d_rec, d_st):
            d.free()


if __name__ == "__main__":
    main()
