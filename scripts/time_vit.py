#!/usr/bin/env python3
"""One call of the Viterbi decoder (sfe_dsp_vit_*): n_bursts rows of float32 soft values in HBM -- terminated bursts of BPSK
at Eb/N0 = 3 dB, every row its own noise -- into payload bytes, records and statuses:
    ours   sfe_dsp_vit_process_stream: HIP events, 20 warm-up calls, then 5 windows of 200 calls each: the median window's
           mean per call, with the fastest and the slowest window beside it.  Nothing synchronises inside a window.  The
           input is the same buffer in every call (at most 8.6 MB: it stays in the last-level cache).
Beside each row, in the same process, the two compositions it replaces:
    torch  the same law composed of torch-ROCm tensor operations over the same device buffer, all bursts at once: the
           2^n branch sums of every step in one batched pass, then per step two gathers of the metrics, two of the branch
           sums, two additions, a comparison and a select, and per traceback step a gather and the shifts -- about fifteen
           launches per trellis step (the finite check and the packing are left out, in torch's favour); HIP events, 1
           warm-up call, then 3 windows of 1 call, median and range as above.  Its bits are compared with the block's.
    host   the round trip: copy the soft values down, sfe_dsp_vit_plan (float32 on one host core), copy the bytes up;
           wall clock, one warm-up then 3 calls, median and range.
The check column compares the first four bursts with the plan's bytes, metric words and counts, and counts the payload bits
the call decoded wrongly.
    python scripts/time_vit.py > profiles/vit/time_vit.txt
TORCH=0 leaves the torch composition out; SHAPES="K:n:n_info:n_bursts:punctured;..." limits the run to those rows."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api, synth  # noqa: E402

WARM, WINDOWS, REPS, TORCH_WARM, TORCH_WINDOWS, TORCH_REPS, HOST_REPS, CHECK = 20, 5, 200, 1, 3, 1, 3, 4
TORCH = os.environ.get("TORCH", "1") != "0"
GEN = {(7, 2): (0o171, 0o133), (9, 2): (0o561, 0o753)}
PUNCT = [[1, 1], [1, 0], [0, 1]]            # rate 3/4
SHAPES = [(7, 2, 256, 1, 0), (7, 2, 256, 4096, 0), (7, 2, 8192, 256, 0), (9, 2, 2048, 256, 0), (7, 2, 256, 4096, 1)]
WANT = {tuple(int(v) for v in s.split(":")) for s in os.environ["SHAPES"].split(";")} if os.environ.get("SHAPES") else None


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


def torch_law(torch, X, K, gen, keep, n_info):
    """The law on a (n_bursts, n_soft) float32 tensor of terminated bursts: the decoded bits, (n_bursts, n_info) uint8."""
    nb, dev, n, S = X.shape[0], X.device, len(gen), 1 << (K - 1)
    T = n_info + K - 1
    keep = np.ones((1, n), bool) if keep is None else np.asarray(keep, bool)
    mask = np.array([keep[t % len(keep)] for t in range(T)]).ravel()
    R = torch.zeros((nb, T * n), dtype=torch.float32, device=dev)
    R[:, torch.as_tensor(np.flatnonzero(mask), device=dev)] = X
    R = R.reshape(nb, T, n)
    labels = np.arange(1 << n)
    BM = None                                                       # (nb, T, 2^n): ((+-r_0) + (+-r_1)) + ...
    for j in range(n):
        sign = torch.as_tensor(np.where((labels >> j) & 1, -1.0, 1.0).astype(np.float32), device=dev)
        term = R[:, :, j:j + 1] * sign
        BM = term if BM is None else BM + term
    s = np.arange(S)

    def label(reg):
        return sum(np.array([bin(int(r) & g).count("1") & 1 for r in reg]) << j for j, g in enumerate(gen))
    p0 = torch.as_tensor(s >> 1, device=dev)
    p1 = torch.as_tensor((s >> 1) | (S >> 1), device=dev)
    l0, l1 = torch.as_tensor(label(s), device=dev), torch.as_tensor(label(s | S), device=dev)
    pm = torch.full((nb, S), -float("inf"), dtype=torch.float32, device=dev)
    pm[:, 0] = 0.0
    D = torch.empty((T, nb, S), dtype=torch.bool, device=dev)
    for t in range(T):
        bm = BM[:, t]
        c0, c1 = pm[:, p0] + bm[:, l0], pm[:, p1] + bm[:, l1]
        torch.gt(c1, c0, out=D[t])
        pm = torch.where(D[t], c1, c0)
    st = torch.zeros((nb, 1), dtype=torch.long, device=dev)
    bits = torch.empty((T, nb, 1), dtype=torch.uint8, device=dev)
    for t in range(T - 1, -1, -1):
        bits[t] = st & 1
        st = (st >> 1) | (D[t].gather(1, st).long() << (K - 2))
    return bits[:n_info, :, 0].T


def main():
    torch = None
    if TORCH:
        import torch
        print(f"# torch {torch.__version__}")
    print("# terminated bursts, BPSK at Eb/N0 = 3 dB, float32 soft input; ms per call; Mbit/s of decoded payload")
    print(f"{'K':>1s} {'n':>1s} {'n_info':>6s} {'bursts':>6s} {'punct':>5s} {'ms':>9s} {'min':>7s} {'max':>7s} {'Mbit/s':>8s} {'torch ms':>9s} {'min':>8s} {'max':>8s} "
          f"{'x':>8s} {'host ms':>9s} {'min':>8s} {'max':>8s} {'x':>8s}   check")
    lib = api._l.load()
    for K, n, n_info, nb, punct in SHAPES:
        if WANT is not None and (K, n, n_info, nb, punct) not in WANT:
            continue
        gen, keep = GEN[(K, n)], PUNCT if punct else None
        bits = synth.vit_bits(n_info, synth.SEED + n_info)
        coded = api.vit_encode(K, gen, bits, keep)
        rate = n_info / coded.size
        x = synth.vit_soft(np.tile(coded, (nb, 1)), 3.0, rate, seed=synth.SEED + nb)
        h = api.Vit(K, gen, n_info, keep)
        d_x = api.DeviceArray.from_numpy(x)
        d_by, d_rec, d_st = api.DeviceArray((nb * h.n_bytes + 3) // 4), api.DeviceArray(2 * nb), api.DeviceArray(nb)
        ms, lo, hi = time_calls(lambda: h.process_stream(d_x, nb, d_by, d_rec, d_st), WARM, WINDOWS, REPS)
        api.sync()
        by = d_by.to_numpy().view(np.uint8)[:nb * h.n_bytes].reshape(nb, h.n_bytes)
        rec, st = d_rec.to_numpy().view(np.uint32).reshape(nb, 2), d_st.to_numpy().view(np.int32)
        k = min(nb, CHECK)
        pby, prec, pst = api.vit_plan(K, gen, n_info, keep, x=x[:k])
        equal = np.array_equal(by[:k], pby) and np.array_equal(rec[:k], prec) and np.array_equal(st[:k], pst)
        wrong = int(np.unpackbits(by ^ synth.vit_pack(bits)[None, :], axis=1).sum())
        chk = f"status {int(st.max())}, first {k} bursts {'equal' if equal else 'DIFFER from'} the plan's, {wrong} of {nb * n_info} payload bits wrong"
        h.close()

        tnote = f"{'':>9s} {'':>8s} {'':>8s} {'':>8s}"
        if torch is not None:
            try:
                dev = torch.device("cuda:0")
                X = torch.as_tensor(_Cai(d_x.ptr, (nb, x.shape[1]), "<f4"), device=dev)
                last = []

                def run():
                    last[:] = [torch_law(torch, X, K, gen, keep, n_info)]
                tm, tlo, thi = time_calls(run, TORCH_WARM, TORCH_WINDOWS, TORCH_REPS)
                torch.cuda.synchronize()
                tnote = f"{tm:9.2f} {tlo:8.2f} {thi:8.2f} {tm / ms:8.1f}"
                tb = np.packbits(last[0].cpu().numpy(), axis=1)
                chk += f"; torch's bits {'equal' if np.array_equal(tb, by) else 'DIFFER'}"
                del X, last
                torch.cuda.empty_cache()
            except Exception as e:
                tnote = f"{'n/a':>9s} {'':>8s} {'':>8s} {'':>8s}"
                chk += f"; torch: {type(e).__name__}: {str(e)[:60]}"

        host, up = np.empty_like(x), np.zeros(((nb * h.n_bytes + 3) // 4) * 4, np.uint8)

        def round_trip():
            api.check(lib.sfe_dsp_memcpy_d2h(host.ctypes.data, d_x.ptr, host.nbytes, None))
            api.sync()
            got = api.vit_plan(K, gen, n_info, keep, x=host)[0]
            up[:got.size] = got.ravel()
            api.check(lib.sfe_dsp_memcpy_h2d(d_by.ptr, up.ctypes.data, up.nbytes, None))
            api.sync()
        round_trip()
        ths = []
        for _ in range(HOST_REPS):
            t0 = time.perf_counter()
            round_trip()
            ths.append((time.perf_counter() - t0) * 1e3)
        th = float(np.median(ths))
        print(f"{K:1d} {n:1d} {n_info:6d} {nb:6d} {punct:5d} {ms:9.4f} {lo:7.4f} {hi:7.4f} {nb * n_info / ms / 1e3:8.1f} {tnote} {th:9.3f} {min(ths):8.3f} {max(ths):8.3f} "
              f"{th / ms:8.1f}   {chk}", flush=True)
        for d in (d_x, d_by, d_rec, d_st):
            d.free()


if __name__ == "__main__":
    main()
