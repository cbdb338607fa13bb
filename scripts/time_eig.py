#!/usr/bin/env python3
"""One update of the eigen-decomposition / MUSIC direction finder (sfe_dsp_eig_*): M Gram matrices of (2S)^2 float32 in HBM
into eigenvalues, the null spectrum of B scan vectors and the E = min(S, 2) leading eigen-beams, signal_dim = 2, in both
modes (the linear one decomposes the S x S Hermitian matrix, the widely-linear one the 2S x 2S real matrix):
    ours   sfe_dsp_eig_process_stream: HIP events, 5 warm-up updates then 20 timed ones, mean.  Nothing synchronises
           inside the loop.
Beside each row, in the same process, the two compositions it replaces:
    torch  torch-ROCm's batched torch.linalg.eigh over the same device buffer (the real 2S x 2S matrices as they lie: the
           widely-linear problem; the structure, the null spectrum and the repack are left out, in torch's favour); HIP
           events, 2 warm-up then 5 timed calls.  Its eigenvalues of band 0 are compared with the block's.
    host   the round trip: copy the matrices down, sfe_dsp_eig_plan (float64 on one host core, widely-linear mode); wall
           clock, one update (256 matrices of order 128 take most of a minute).
The check column compares the eigenvalues of the first four bands with the plan's.
    python scripts/time_eig.py > profiles/eig/time_eig.txt
TORCH=0 leaves the torch composition out; SHAPES="S:B:M;..." limits the run to those rows."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api  # noqa: E402

WARM, REPS, TORCH_REPS, CHECK_BANDS = 5, 20, 5, 4
TORCH = os.environ.get("TORCH", "1") != "0"
SHAPES = [(4, 1, 1), (16, 16, 1), (64, 64, 1), (8, 8, 256), (64, 64, 256)]
WANT = {tuple(int(v) for v in s.split(":")) for s in os.environ["SHAPES"].split(";")} if os.environ.get("SHAPES") else None
SIGNAL_DIM = 2


def time_calls(run, warm, reps):
    t = api.Timer()
    for _ in range(warm):
        run()
    t.start()
    for _ in range(reps):
        run()
    t.stop()
    return t.elapsed_ms() / reps


class _Cai:
    """A window of a DeviceArray for torch.as_tensor (the CUDA array interface, which torch-ROCm reads too)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def problems(S, M, rng):
    """(M, 2S, 2S) float32 Gram matrices of 8S instants of S streams: a strong common component and unit noise."""
    n = 2 * S
    U = rng.standard_normal((M, n, 4 * n)) + 3.0 * rng.standard_normal((M, 1, 4 * n))
    return (np.matmul(U, U.transpose(0, 2, 1)) / (4 * n)).astype(np.float32)


def main():
    rng = np.random.default_rng(11)
    torch = None
    if TORCH:
        import torch
        print(f"# torch {torch.__version__}")
    print("# signal_dim = %d, n_vec = min(S, 2); ms per update" % SIGNAL_DIM)
    print(f"{'S':>3s} {'B':>3s} {'M':>4s} {'linear ms':>10s} {'wl ms':>9s} {'torch ms':>9s} {'x wl':>7s} {'host ms':>9s} {'x wl':>8s}   check")
    for S, B, M in SHAPES:
        if WANT is not None and (S, B, M) not in WANT:
            continue
        n, E = 2 * S, min(S, 2)
        G = problems(S, M, rng)
        u = -1.0 + (2.0 * np.arange(B) + 1.0) / B
        st = np.broadcast_to(np.exp(1j * np.pi * u[:, None] * np.arange(S)[None, :]).astype(np.complex64), (M, B, S)).copy()
        d_g, d_v = api.DeviceArray.from_numpy(G.ravel()), api.DeviceArray(M * n)
        d_n, d_e, d_s = api.DeviceArray(M * B), api.DeviceArray(M * 2 * E * n), api.DeviceArray(M)
        ms, chk = {}, ""
        for wl in (False, True):
            eg = api.Eig(st, wl, SIGNAL_DIM, E)
            ms[wl] = time_calls(lambda: eg.process_stream(d_g, 1, d_v, d_n, d_e, d_s), WARM, REPS)
            api.sync()
            val, status = d_v.to_numpy().reshape(M, n), d_s.to_numpy().view(np.int32)
            k = min(M, CHECK_BANDS)
            vp, _, _, sp = api.eig_plan(st[:k], G[:k], wl, SIGNAL_DIM, E)
            chk += f"{'wl' if wl else 'linear'}: status {int(status.max())}/{int(sp.max())}, max |values - plan| / lambda_0 {np.abs(val[:k] - vp).max() / vp.max():.1e}; "
            eg.close()
        val_wl = val

        tnote = f"{'':>9s} {'':>7s}"
        if torch is not None:
            try:
                dev = torch.device("cuda:0")
                Gt = torch.as_tensor(_Cai(d_g.ptr, (M, n, n), "<f4"), device=dev)
                last = []

                def run():
                    last[:] = [torch.linalg.eigh(Gt)]
                tm = time_calls(run, 2, TORCH_REPS)
                torch.cuda.synchronize()
                lt = last[0][0][0].cpu().numpy()[::-1]
                tnote = f"{tm:9.3f} {tm / ms[True]:7.2f}"
                chk += f"max |values - torch's| / lambda_0 of band 0 {np.abs(lt - val_wl[0]).max() / lt.max():.1e}"
                del Gt, last
                torch.cuda.empty_cache()
            except Exception as e:          # a torch build without a batched eigh for this device
                tnote = f"{'n/a':>9s} {'':>7s}"
                chk += f"torch: {type(e).__name__}: {str(e)[:60]}"

        host = np.empty_like(G)

        def round_trip():
            api.check(api._l.load().sfe_dsp_memcpy_d2h(host.ctypes.data, d_g.ptr, host.nbytes, None))
            api.sync()
            api.eig_plan(st, host, True, SIGNAL_DIM, E)
        t0 = time.perf_counter()
        round_trip()
        th = (time.perf_counter() - t0) * 1e3
        print(f"{S:3d} {B:3d} {M:4d} {ms[False]:10.4f} {ms[True]:9.4f} {tnote} {th:9.3f} {th / ms[True]:8.1f}   {chk}", flush=True)
        for d in (d_g, d_v, d_n, d_e, d_s):
            d.free()


if __name__ == "__main__":
    main()
