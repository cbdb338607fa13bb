"""What the Viterbi-decoder tests share (tests/test_vit_host.py, tests/test_gpu_vit.py, tests/test_gpu_vit_grid.py): the
law restated in numpy float32, the rows of soft values, the guarded call, and the grid of codes, puncturing patterns and
sizes that launches every kernel class.  Host only at import: numpy and simplefe_amd.synth; what needs the library or a
GPU takes `api` as an argument."""
import numpy as np

from simplefe_amd import synth

F32 = np.float32
SENT = np.float32(-7654.25)         # around records and statuses
SENT_BYTE = 0xA5                    # around the payload bytes


# ---- the law, restated: nothing below calls the library
def parity(v):
    v = np.asarray(v, np.uint32).copy()
    for sh in (16, 8, 4, 2, 1):
        v ^= v >> sh
    return (v & 1).astype(np.uint8)


def encode_np(K, gen, bits, keep=None, terminated=True):
    """(the kept coded bits, every coded bit as (T, n), the (T, n) mask of kept positions)."""
    n = len(gen)
    word = list(bits) + [0] * (K - 1 if terminated else 0)
    keep = np.ones((1, n), np.uint8) if keep is None else np.asarray(keep, np.uint8)
    s, full = 0, np.zeros((len(word), n), np.uint8)
    for t, u in enumerate(word):
        reg = ((s << 1) | int(u)) % (1 << K)
        for j, g in enumerate(gen):
            full[t, j] = bin(reg & g).count("1") & 1
        s = reg % (1 << (K - 1))
    mask = np.array([keep[t % len(keep)] for t in range(len(word))], bool)
    return full[mask], full, mask


def law_np(K, gen, n_info, soft, keep=None, terminated=True):
    """One burst by the law of include/sfe_dsp.h in numpy float32: (bytes uint8, metric word uint32, count, status)."""
    n, S = len(gen), 1 << (K - 1)
    T = n_info + (K - 1 if terminated else 0)
    soft = np.asarray(soft, F32)
    nbytes = (n_info + 7) // 8
    if not np.isfinite(soft).all():
        return np.zeros(nbytes, np.uint8), 0x7fc00000, 0, 1
    keep = np.ones((1, n), np.uint8) if keep is None else np.asarray(keep, np.uint8)
    r = np.zeros((T, n), F32)                   # punctured positions: +0
    i = 0
    for t in range(T):
        for j in range(n):
            if keep[t % len(keep), j]:
                r[t, j] = soft[i]
                i += 1
    assert i == soft.size
    s = np.arange(S)
    p0, p1 = s >> 1, (s >> 1) | (S >> 1)
    u = s & 1
    regs = [(p << 1 | u) % (1 << K) for p in (p0, p1)]
    neg = [[parity(reg & g).astype(bool) for g in gen] for reg in regs]      # [branch][j][state]
    pm = np.full(S, -np.inf, F32)
    pm[0] = F32(0.0)
    dec = np.zeros((T, S), np.uint8)
    for t in range(T):
        cand = []
        for br, p in enumerate((p0, p1)):
            bm = np.where(neg[br][0], -r[t, 0], r[t, 0]).astype(F32)
            for j in range(1, n):
                bm = (bm + np.where(neg[br][j], -r[t, j], r[t, j]).astype(F32)).astype(F32)
            cand.append((pm[p] + bm).astype(F32))
        dec[t] = cand[1] > cand[0]
        pm = np.where(dec[t].astype(bool), cand[1], cand[0]).astype(F32)
    end = 0 if terminated else int(np.argmax(pm))           # the first of the largest
    word, st = np.zeros(T, np.uint8), end
    for t in range(T - 1, -1, -1):
        word[t] = st & 1
        st = (st >> 1) | (int(dec[t, st]) << (K - 2))
    bits = word[:n_info]
    _, full, mask = encode_np(K, gen, bits, keep, terminated)
    count = int((((full == 1) & (r > 0)) | ((full == 0) & (r < 0)))[mask].sum())
    return np.packbits(bits), int(pm[end:end + 1].view(np.uint32)[0]), count, 0


def soft_inputs(K, gen, n_info, keep, terminated, seed):
    """Three rows of a shape: noisy BPSK at 2 dB, integer-valued values (most steps tie), all zeros."""
    bits = synth.vit_bits(n_info, seed)
    coded = encode_np(K, gen, bits, keep, terminated)[0]
    rng = np.random.default_rng(seed + 1)
    noisy = synth.vit_soft(coded, 2.0, 1.0 / len(gen), seed + 2)
    ints = rng.integers(-2, 3, size=coded.size).astype(F32)
    return np.stack([noisy, ints, np.zeros(coded.size, F32)])


# ---- on the GPU: rows of soft values and one call through guarded buffers
def rows_of(api, K, gen, n_info, keep, terminated, n_bursts, seed):
    """n_bursts rows of soft values: noisy BPSK at 2 dB of different payloads, and, as rows 1 and 2 (where there are that
    many), integer-valued values -- most steps tie -- and all zeros."""
    rng = np.random.default_rng(seed)
    rows = []
    for b in range(n_bursts):
        coded = api.vit_encode(K, gen, synth.vit_bits(n_info, seed + 10 * b), keep, terminated)
        if b == 1:
            rows.append(rng.integers(-2, 3, size=coded.size).astype(F32))
        elif b == 2:
            rows.append(np.zeros(coded.size, F32))
        else:
            rows.append(synth.vit_soft(coded, 2.0, 1.0 / len(gen), seed + 10 * b + 1))
    return np.stack(rows)


def run(api, h, x, in_pad=0, out_pad=0, lead=0, status_in=None, call=None):
    """One call through guarded buffers: the rows `lead` elements into their buffer and in_pad elements apart, the bytes
    out_pad apart, a sentinel everywhere else; returns (bytes, record, status) with the guard bands checked.  `call`
    replaces the plain process_stream (a captured one, say): it gets the same arguments."""
    soft = h.in_mode == 0
    x = np.ascontiguousarray(x, F32 if soft else np.complex64)
    nb, w = x.shape[0], 1 if soft else 2
    stride = x.shape[1] + in_pad
    buf = np.full((lead + nb * stride + 3) * w, np.nan, F32)
    for b in range(nb):
        buf[(lead + b * stride) * w:][:x.shape[1] * w] = x[b].view(F32)
    d_in = api.DeviceArray.from_numpy(buf)
    ostride, front = h.n_bytes + out_pad, 5
    raw_by = np.full(front + nb * ostride + 7, SENT_BYTE, np.uint8)
    d_by = api.DeviceArray.from_bytes(raw_by)
    d_rec, d_st = api.DeviceArray.from_numpy(np.full(3 + 2 * nb + 5, SENT, F32)), api.DeviceArray.from_numpy(np.full(5 + nb + 3, SENT, F32))
    held = [d_in, d_by, d_rec, d_st]
    d_si = None
    if status_in is not None:
        d_si = api.DeviceArray.from_numpy(np.ascontiguousarray(status_in, np.int32).view(F32))
        held.append(d_si)
    try:
        args = (d_in.ptr + 4 * w * lead, nb, d_by.ptr + front, d_rec.ptr + 12, d_st.ptr + 20, d_si)
        k = (call or h.process_stream)(*args, in_stride=stride, out_stride=ostride)
        api.sync()
        assert k == nb
        by, rec, st = d_by.to_numpy().view(np.uint8)[:raw_by.size], d_rec.to_numpy(), d_st.to_numpy()
    finally:
        for d in held:
            d.free()
    sent = np.array([SENT]).view(np.uint32)[0]
    body = by[front:front + nb * ostride].reshape(nb, ostride)
    assert (by[:front] == SENT_BYTE).all() and (by[front + nb * ostride:] == SENT_BYTE).all() and (body[:, h.n_bytes:] == SENT_BYTE).all()
    assert (rec[:3].view(np.uint32) == sent).all() and (rec[3 + 2 * nb:].view(np.uint32) == sent).all()
    assert (st[:5].view(np.uint32) == sent).all() and (st[5 + nb:].view(np.uint32) == sent).all()
    return np.ascontiguousarray(body[:, :h.n_bytes]), rec[3:3 + 2 * nb].view(np.uint32).reshape(nb, 2), st[5:5 + nb].view(np.int32)


def same(got, want):
    return all(np.array_equal(u, v) for u, v in zip(got, want))


# ---- the grid: every (n_gen, states per lane) class of the kernel, idle lanes (K <= 6), both words of the keep mask
# K: its first 2, 3 and 4 generators make the grid's 21 codes
GENS = {3: (7, 5, 7, 6), 4: (0o17, 0o13, 0o15, 0o11), 5: (0o23, 0o35, 0o27, 0o33), 6: (0o53, 0o75, 0o65, 0o47),
        7: (0o171, 0o133, 0o165, 0o117), 8: (0o247, 0o371, 0o225, 0o331), 9: (0o561, 0o753, 0o711, 0o663)}
GRID_CODES = [(K, GENS[K][:n]) for K in sorted(GENS) for n in (2, 3, 4)]
GRID_CODE_IDS = ["K%dn%d" % (K, len(g)) for K, g in GRID_CODES]
# rate-3/4 patterns of period 3: four of a period's positions are kept (n = 2: the usual one)
PUNCT3 = {2: [[1, 1], [1, 0], [0, 1]], 3: [[1, 1, 0], [1, 0, 0], [0, 0, 1]], 4: [[1, 1, 0, 0], [1, 0, 1, 0], [0, 0, 0, 0]]}
GRID_SIZES = (1, 40, 131)           # 131 + K - 1 steps: a partial last period for P = 17 and P = 32, two 64-step boundaries
KEEP_SEED = 1732


def mask_words(keep):
    """The two 64-bit words of a pattern as the block packs them: bit 4 (t mod P) + j is set where keep[t mod P][j]."""
    m = 0
    for tp, row in enumerate(keep):
        for j, v in enumerate(row):
            m |= int(v) << (4 * tp + j)
    return m & (2 ** 64 - 1), m >> 64


def long_pattern(P, n):
    """A fixed-seed pattern of period P (17 or 32) with about 60 % kept: its first position kept, its last one kept, and
    of step 16 -- mask bits 64 .. 64 + n - 1, the first of the second word -- generator 0 kept and generator n - 1 not
    (at P = 17 step 16 is the last step, and the later rule holds)."""
    rng = np.random.default_rng(KEEP_SEED + 100 * P + n)
    keep = (rng.random((P, n)) < 0.6).astype(np.uint8)
    keep[0][0] = 1
    keep[P - 1][n - 1] = 1
    keep[16][0] = 1
    keep[16][n - 1] = 0
    return keep.tolist()


LONG = {(P, n): long_pattern(P, n) for P in (17, 32) for n in (2, 3, 4)}
for (_P, _n), _keep in LONG.items():
    _lo, _hi = mask_words(_keep)
    assert _lo and _hi and (_hi & 1) and not (_hi >> (_n - 1)) & 1, (_P, _n)         # both words; bit 64 kept; both kinds behind it
    assert _P == 17 or _hi >> 1, (_P, _n)               # a kept position behind bit 64: its index counts all of the first word
    assert 0.4 <= np.mean(_keep) <= 0.8, (_P, _n)


def patterns(n):
    """(name, keep) of the grid's four patterns for n generators."""
    return [("all", None), ("p3", PUNCT3[n]), ("p17", LONG[17, n]), ("p32", LONG[32, n])]


def grid_cases(K, gen):
    """Every (pattern name, keep, terminated, n_info, seed) of one code: 4 patterns x 2 endings x 3 sizes."""
    out = []
    for pi, (name, keep) in enumerate(patterns(len(gen))):
        for terminated in (True, False):
            for n_info in GRID_SIZES:
                out.append((name, keep, terminated, n_info, 1000 * K + 100 * len(gen) + 10 * pi + n_info))
    return out
