"""What tests/test_mod_host.py and tests/test_gpu_mod.py share: the codes, the shapes of the grid, and the loopback chain's
shape -- the CHAIN of tests/test_gpu_vit.py with a raised-cosine pulse cut at +-8 symbols in front of it."""
import numpy as np

from simplefe_amd import synth

F32 = np.float32
# (K, generators): the codes of tests/test_vit_host.py and one of four generators
CODES = [(3, (7, 5)), (7, (0o171, 0o133)), (7, (0o133, 0o171, 0o165)), (8, (0o247, 0o371)), (9, (0o561, 0o753)),
         (9, (0o765, 0o671, 0o513, 0o473))]
CODE_IDS = ["K3", "K7", "K7n3", "K8", "K9", "K9n4"]
# rate-3/4 patterns of period 3: four of a period's positions are kept
PUNCT = {2: [[1, 1], [1, 0], [0, 1]], 3: [[1, 1, 0], [1, 0, 0], [0, 0, 1]], 4: [[1, 1, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0]]}

CHAIN = dict(sps=10, N=256, Lp=32, lag=4, K=7, gen=(0o171, 0o133), n_info=106, n_taps=161, Q=17, F=2720, amp=0.5, step=3584, base=100,
             n_bursts=4, tpl_at=80, tpl_len=311, min_energy=1e-3)


def payload_bytes(n_info, n_bursts, seed):
    """(n_bursts, ceil(n_info / 8)) random bytes: the pad bits of the last byte are random too (the law ignores them)."""
    return np.random.default_rng(seed).integers(0, 256, size=(int(n_bursts), (int(n_info) + 7) // 8), dtype=np.uint8)


def payload_bits(data, n_info):
    """The n_info payload bits of one burst's bytes, MSB-first."""
    return np.unpackbits(np.asarray(data, np.uint8).ravel())[:int(n_info)]


def rc_taps(sps, span):
    """A raised cosine cut at +-span symbols, 2 span sps + 1 taps, float32: symbol k peaks at frame sample k sps + span sps."""
    return synth.raised_cosine(np.arange(-span * sps, span * sps + 1) / float(sps)).astype(F32)


def chain_parts():
    """(taps, preamble complex64, payload bytes (4, 14), the correlator's template complex64 (311,)) of the loopback."""
    c = CHAIN
    taps = rc_taps(c["sps"], 8)
    pre = synth.psk_symbols(c["Lp"], 4, seed=synth.SEED + 3).astype(np.complex64)
    data = payload_bytes(c["n_info"], c["n_bursts"], 900)
    data[:, -1] &= 0xC0                                          # 106 = 13 * 8 + 2: the decoder writes pad bits of 0
    # a preamble-only frame, from symbol 0's peak to symbol 31's
    frame = synth.mod_reference(synth.mod_symbols([], 2, c["amp"], pre), taps, c["sps"])
    tpl = frame[c["tpl_at"]:c["tpl_at"] + c["tpl_len"]].astype(np.complex64)
    assert taps.size == c["n_taps"] and tpl.size == c["tpl_len"]
    return taps, pre, data, tpl


def chain_plan_kwargs():
    c = CHAIN
    return dict(K=c["K"], gen=c["gen"], n_info=c["n_info"], sps=c["sps"], order=2, amp=c["amp"])


def tx10_as_u8_samples(tx):
    """The transmit wire format's bytes as the receive wire format's: each 10-bit word decoded and requantised to a byte."""
    return synth.f32_to_u8(synth.tx10_unpack(tx))
