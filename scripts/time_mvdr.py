#!/usr/bin/env python3
"""One weight update of the adaptive beamforming solver (sfe_dsp_mvdr_*): M Gram matrices of (2S)^2 float32 in HBM into
the beamformer's weight table, widely-linear mode (2B right-hand sides per matrix), load_rel = 1e-2:
    ours   sfe_dsp_mvdr_process_stream + sfe_dsp_mvdr_load_beam on one stream: HIP events, 5 warm-up updates then 20
           timed ones, mean.  Nothing synchronises inside the loop.
Beside each row, in the same process, the two compositions it replaces:
    torch  torch-ROCm over the same device buffer: the loading, batched linalg.cholesky and cholesky_solve of the 2B
           right-hand sides (the 2 x 2 finish and the repack into the weight table are left out, in torch's favour);
           HIP events, 2 warm-up then 5 timed calls.  Its Z of band 0, beam 0 is finished on the host and compared with the block's rows.
    host   the round trip: copy the matrices down, sfe_dsp_mvdr_plan (float64 on one host core), sfe_dsp_beam_set_weights
           (which brackets its upload with two device synchronisations); wall clock, 1 warm-up then 3 timed updates.
    flop = per problem n^3 / 3 (factor) + 4 B n^2 (2B substitutions, both ways), n = 2S
    python scripts/time_mvdr.py > profiles/mvdr/time_mvdr.txt
TORCH=0 leaves the torch composition out; SHAPES="S:B:M;..." limits the run to those rows."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api, synth  # noqa: E402

WARM, REPS, TORCH_REPS, HOST_REPS = 5, 20, 5, 3
TORCH = os.environ.get("TORCH", "1") != "0"
SHAPES = [(4, 1, 1), (16, 16, 1), (64, 64, 1), (8, 8, 256), (64, 64, 256)]
WANT = {tuple(int(v) for v in s.split(":")) for s in os.environ["SHAPES"].split(";")} if os.environ.get("SHAPES") else None
LOAD_REL = 1e-2


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


def weights_of(R):
    """(W, V) of real matrices (M, 2B, 2S): the inverse of sfe_dsp_beam_plan's map."""
    a, b, c, d = R[:, 0::2, 0::2], R[:, 0::2, 1::2], R[:, 1::2, 0::2], R[:, 1::2, 1::2]
    return ((a + d) + 1j * (c - b)) / 2, ((a - d) + 1j * (c + b)) / 2


def main():
    rng = np.random.default_rng(11)
    torch = None
    if TORCH:
        import torch
        print(f"# torch {torch.__version__}")
    print("# widely-linear mode, load_rel = %g; ms per update" % LOAD_REL)
    print(f"{'S':>3s} {'B':>3s} {'M':>4s} {'ours ms':>9s} {'MFLOP':>8s} {'GFLOP/s':>8s} {'torch ms':>9s} {'x':>7s} {'host ms':>9s} {'x':>8s}   check")
    for S, B, M in SHAPES:
        if WANT is not None and (S, B, M) not in WANT:
            continue
        n = 2 * S
        G = problems(S, M, rng)
        u = -1.0 + (2.0 * np.arange(B) + 1.0) / B
        st = np.broadcast_to(np.exp(1j * np.pi * u[:, None] * np.arange(S)[None, :]).astype(np.complex64), (M, B, S)).copy()
        mv, beam = api.Mvdr(st, True, LOAD_REL), api.Beam(np.zeros((M, B, S), np.complex64))
        d_g, d_R = api.DeviceArray.from_numpy(G.ravel()), api.DeviceArray(M * 2 * B * n)
        d_p, d_s = api.DeviceArray(M * B), api.DeviceArray(M)

        def update():
            mv.process_stream(d_g, 1, d_R, d_p, d_s)
            mv.load_beam(beam, d_R)
        ms = time_calls(update, WARM, REPS)
        api.sync()
        R = d_R.to_numpy().reshape(M, 2 * B, n)
        status = d_s.to_numpy().view(np.int32)
        Rp, _, sp = api.mvdr_plan(st, G, True, LOAD_REL)
        chk = f"status {int(status.max())}/{int(sp.max())}, |R - plan| / |plan| {np.linalg.norm(R - Rp) / np.linalg.norm(Rp):.1e}"
        mflop = M * (n ** 3 / 3.0 + 4.0 * B * n * n) / 1e6

        tnote = f"{'':>9s} {'':>7s}"
        if torch is not None:
            try:
                dev = torch.device("cuda:0")
                Gt = torch.as_tensor(_Cai(d_g.ptr, (M, n, n), "<f4"), device=dev)
                A2 = torch.as_tensor(np.stack([np.concatenate([synth.mvdr_rhs(st[k, b], np.float32) for b in range(B)], axis=1)
                                               for k in range(M)]), device=dev)
                eye = torch.eye(n, device=dev)
                last = []

                def run():
                    lam = LOAD_REL * torch.diagonal(Gt, dim1=1, dim2=2).sum(1) / n
                    Lt = torch.linalg.cholesky(Gt + lam[:, None, None] * eye)
                    last[:] = [torch.cholesky_solve(A2, Lt)]
                tm = time_calls(run, 2, TORCH_REPS)
                torch.cuda.synchronize()
                Z = last[0][0].cpu().numpy().astype(np.float64)                 # band 0: (n, 2B)
                Rt = np.linalg.solve(A2[0, :, :2].cpu().numpy().astype(np.float64).T @ Z[:, :2], Z[:, :2].T)    # Q^-1 Z^T of beam 0
                tnote = f"{tm:9.3f} {tm / ms:7.2f}"
                chk += f", |R - torch's| / |R| of beam 0 {np.linalg.norm(Rt - R[0, :2]) / np.linalg.norm(Rt):.1e}"
                del Gt, A2, last
                torch.cuda.empty_cache()
            except Exception as e:          # a torch build without a batched Cholesky for this device
                tnote = f"{'n/a':>9s} {'':>7s}"
                chk += f", torch: {type(e).__name__}: {str(e)[:60]}"

        host = np.empty_like(G)

        def round_trip():
            api.check(api._l.load().sfe_dsp_memcpy_d2h(host.ctypes.data, d_g.ptr, host.nbytes, None))
            api.sync()
            W, V = weights_of(api.mvdr_plan(st, host, True, LOAD_REL)[0])
            beam.set_weights(W, V)
        round_trip()
        t0 = time.perf_counter()
        for _ in range(HOST_REPS):
            round_trip()
        th = (time.perf_counter() - t0) * 1e3 / HOST_REPS
        print(f"{S:3d} {B:3d} {M:4d} {ms:9.4f} {mflop:8.2f} {mflop / ms:8.1f} {tnote} {th:9.3f} {th / ms:8.1f}   {chk}", flush=True)
        for d in (d_g, d_R, d_p, d_s):
            d.free()
        mv.close()
        beam.close()


if __name__ == "__main__":
    main()
