"""One call of the OFDM receiver through guarded device buffers, shared by tests/test_gpu_ofdm.py and
tests/test_gpu_ofdm_grid.py.  Nothing here touches the library or a GPU at import: `api` is an argument."""
import numpy as np

F32 = np.float32
SENT = np.float32(-7654.25)


def _bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


def same(a, b):
    return all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a, b))


class Run:
    """One call's buffers with room around every output: the input rows `lead` samples into their buffer, outputs with
    strides wider than their payload, a sentinel everywhere else.  launch() may be called again (a captured stream)."""

    def __init__(self, api, h, x, n_bursts, idx=None, gate=None, out_pad=0, st_pad=0, lead=0, in_pad=0, start_base=0, start_step=0,
                 chan=True, stream=None, launch=True):
        self.api, self.h, S, M = api, h, h.n_streams, h.n_sym
        x = np.asarray(x).reshape(S, -1)
        self.u8 = x.dtype == np.uint8
        self.n_in = x.shape[1] // 2 if self.u8 else x.shape[1]
        row = x if self.u8 else x.astype(np.complex64).view(F32)
        self.in_stride = self.n_in + in_pad
        buf = np.full(2 * lead + S * self.in_stride * 2 + 8, 0x55 if self.u8 else np.nan, row.dtype)
        for s in range(S):
            buf[2 * lead + s * self.in_stride * 2:][:self.n_in * 2] = row[s]
        self.d_in = api.DeviceArray.from_bytes(buf) if self.u8 else api.DeviceArray.from_numpy(buf)
        self.in_ptr = self.d_in.ptr + lead * (2 if self.u8 else 8)
        self.nb, self.out_stride, self.st_stride = n_bursts, M + out_pad, n_bursts + st_pad
        self.held = [self.d_in]
        self.d_idx = self.d_gate = None
        if idx is not None:
            self.d_idx = api.DeviceArray.from_numpy(np.ascontiguousarray(idx, np.uint32).reshape(S, n_bursts).view(F32))
            self.held.append(self.d_idx)
        if gate is not None:
            self.d_gate = api.DeviceArray.from_numpy(np.ascontiguousarray(gate, F32).reshape(S, n_bursts))
            self.held.append(self.d_gate)
        rows = S * n_bursts
        # floats before each output's first slot (symbols and H stay 8-byte aligned), its payload, floats after it
        self.lead = (4, 6, 3, 5)
        self.size = (rows * self.out_stride * 2, rows * h.n_fft * 2, rows * 8, S * self.st_stride)
        self.d = [api.DeviceArray(a + n + 7) for a, n in zip(self.lead, self.size)]
        self.held += self.d
        self.chan, self.base, self.step, self.stream = chan, start_base, start_step, stream
        self.poison()
        if launch:
            self.launch()
            api.sync()

    def poison(self):
        for d in self.d:
            fill = np.full(d.n, SENT, F32)              # alive until the copy has been waited for
            self.api.check(d._L.sfe_dsp_memcpy_h2d(d.ptr, fill.ctypes.data, fill.nbytes, None))
            self.api.sync()

    def launch(self):
        p = [d.ptr + 4 * a for d, a in zip(self.d, self.lead)]
        self.k = self.h.process_stream(self.in_ptr, self.n_in, self.nb, p[0], self.d_idx, self.d_gate, p[1] if self.chan else None, p[2], p[3],
                                       self.base, self.step, in_stride=self.in_stride, out_stride=self.out_stride, status_stride=self.st_stride,
                                       stream=self.stream)

    def read(self):
        """(symbols (S, nb, Ns, Nd), chan (S, nb, N), records (S, nb, 8), statuses (S, nb)), the guard bands checked."""
        h, S, nb, M = self.h, self.h.n_streams, self.nb, self.h.n_sym
        assert self.k == nb
        sent = _bits(np.array([SENT]))[0]
        raw = [d.to_numpy() for d in self.d]
        body = []
        for r, a, n in zip(raw, self.lead, self.size):
            assert (_bits(r[:a]) == sent).all() and (_bits(r[a + n:]) == sent).all()
            body.append(r[a:a + n])
        out = body[0].reshape(S * nb, self.out_stride * 2)
        st = body[3].reshape(S, self.st_stride)
        assert (_bits(out[:, 2 * M:]) == sent).all() and (_bits(st[:, nb:]) == sent).all()
        if not self.chan:
            assert (_bits(body[1]) == sent).all()
        sym = np.ascontiguousarray(out[:, :2 * M]).view(np.complex64).reshape(S, nb, h.n_data, h.n_data_bins)
        return (sym, np.ascontiguousarray(body[1]).view(np.complex64).reshape(S, nb, h.n_fft), body[2].reshape(S, nb, 8),
                np.ascontiguousarray(st[:, :nb]).view(np.int32))

    def free(self):
        for d in self.held:
            d.free()


def run(api, h, x, n_bursts, **kw):
    r = Run(api, h, x, n_bursts, **kw)
    try:
        return r.read()
    finally:
        r.free()
