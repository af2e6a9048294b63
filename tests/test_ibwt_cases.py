"""What the inputs of test_gpu_ibwt.py reach, by the host model of the splitter geometry
(scripts/ibwt_hops.py): the GPU tests name kernel paths -- partial cycles, partial tail stores, the
overflow pool and its exhaustion, both walk verdicts -- and these assertions say that the inputs get
there.  Also pins the oracle's inverse BWT to the reference's on inputs that are no BWT outputs.
CPU only."""
import numpy as np
import pytest

import ibwt_cases as ic
from oracle import Reference, have_ref

model = ic.model
MODEL_MAX = (1 << 20) + 1  # the model runs on every single-block case up to here (S = 64 and S = 128)


@pytest.fixture(scope="module")
def hops():
    """{name: (L, Hops)} of the single-block cases up to MODEL_MAX."""
    return {name: (L, model.hops(L, p)) for name, L, p in ic.single_cases() if L.size <= MODEL_MAX}


def test_geometry_rule():
    # S = 64 up to 16384 splitters, then the next power of two
    assert model.geometry(1) == (6, 1) and model.geometry(65) == (6, 2)
    assert model.geometry(1 << 20) == (6, 16384) and model.geometry((1 << 20) + 1) == (7, 8193)
    assert model.geometry(1 << 21) == (7, 16384) and model.geometry((1 << 21) + 2) == (8, 8193)
    assert model.geometry((1 << 22) + 5) == (9, 8193)
    assert model.pool_capacity(16385) == 2568


def test_model_decodes_like_the_oracle(orc, hops):
    """The model's own hops, chained from the primary splitter and repeated with the cycle length,
    give the oracle's output: the hop lengths, the chain and the cycle are those of the input."""
    seen = 0
    for name, (L, h) in hops.items():
        if h.cycle > 70000:
            continue
        assert int(h.hop_len[h.chain].sum()) == h.cycle and 0 < h.cycle <= h.n, name
        assert model.decode(L, h).tobytes() == orc.bwt_decode(L.tobytes(), h.pi), name
        seen += 1
    assert seen > 200


def test_partial_cycles(hops):
    """Cycles through pi shorter than n that do not divide it (k_ib_chain3 leaves splitters off the
    chain, k_ib_repeat fills with i % c), at S = 64 and S = 128, and cycles of 1 and of 7."""
    partial = {name: h for name, (L, h) in hops.items() if h.cycle < h.n and h.n % h.cycle}
    assert sum(1 for h in partial.values() if h.n == 65536) >= 8
    assert any(h.shift == 7 for h in partial.values())
    for h in partial.values():
        on_chain = np.zeros(h.ns + 1, bool)
        on_chain[h.chain] = True
        if h.n >= 4096 and h.cycle < h.n // 2:
            assert (~on_chain & (h.hop_len > 0)).any()  # walked hops that the chain leaves out
    lengths = {h.cycle for _, h in hops.values()}
    assert 1 in lengths and 7 in lengths
    # one cycle of n in a single hop chain too (a rotation coprime to n)
    assert hops["rotation-n65536-a4099-pi77"][1].cycle == 65536


def test_hop_length_residues_and_overflow(hops):
    """All 16 residues of the hop length mod 16 (store_head's partial tails), among hops that end in
    the first 256 bytes of a slot, in the rest of a slot (S > 64) and in a pool chunk."""
    first, rest, pool = set(), set(), set()
    for _, h in hops.values():
        ln = h.hop_len[h.chain]  # the hops that are copied out
        cap = 4 * h.S
        first |= set((ln[ln <= 256] % 16).tolist())
        rest |= set((ln[(ln > 256) & (ln <= cap)] % 16).tolist())
        pool |= set((ln[ln > cap] % 16).tolist())
    assert first == set(range(16)) and rest == set(range(16)) and pool == set(range(16))
    # hops past the slot at S = 64 and at S = 128
    assert any(h.shift == 6 and h.chunks for _, h in hops.values())
    assert any(h.shift == 7 and h.chunks for _, h in hops.values())


def test_primary_index_positions(hops):
    """The primary index on a regular splitter (no extra hop), off one, and on a fixed point of T."""
    assert any(h.primary < h.ns for _, h in hops.values()) and any(h.primary == h.ns for _, h in hops.values())
    assert any(h.T[h.pi] == h.pi and h.primary == h.ns for _, h in hops.values())
    assert any(h.T[h.pi] == h.pi and h.primary < h.ns for _, h in hops.values())


def test_rotation_closed_forms():
    for n, a, p in ic.ROTATIONS:
        h = model.hops(model.rotation(n, a), p)
        assert np.array_equal(h.T, (np.arange(n) + a) % n)
        assert h.cycle == n // np.gcd(n, a)
    h = model.hops(model.rotation(65536, 2), 12345)
    assert (h.chain.size, int(h.hop_len[h.ns]), h.chunks) == (1, 32768, 127)
    assert h.chunks <= model.pool_capacity(h.nsplit)  # a long overflow chain, no exhaustion


def test_exhausting_rotation():
    """One hop of n / 2 bytes needs more overflow chunks than a context holds that has seen only
    this block; and than a fresh context holds for the three-block batch around it."""
    n, a, p = ic.EXHAUSTING
    h = model.hops(model.rotation(n, a), p)
    assert h.chunks == 4094
    assert h.chunks > (h.ns + 1 + (h.ns + 1) // 8 + 64) // 8 + 256 == model.pool_capacity(h.nsplit)
    pred = ic.predict(ic.exhausting_batch())
    assert pred["chunks"] > pred["fresh_cap"] and pred["walk"] == "two"


def test_walk_verdicts():
    """Both verdicts of k_ib_scan, and every walk mode among the batches."""
    assert model.suits_pairs(ic.random_L(1, 1 << 16, 16)) and not model.suits_pairs(ic.random_L(1, 1 << 16, 256))
    # the rule counts a byte with exactly n / 32 positions as rare
    L = np.repeat(np.arange(32, dtype=np.uint8), 4)
    assert not model.suits_pairs(L)
    L = np.concatenate([np.repeat(np.arange(8, dtype=np.uint8), 4), np.full(97, 9, np.uint8)])  # 32 of 129 rare
    assert model.suits_pairs(L)
    modes = {name: ic.predict(b)["walk"] for name, b in ic.batch_cases().items()}
    assert modes["nine-64k"] == "one" and modes["two-step"] == "two" and modes["one-step-if"] == "one_if"
    assert modes["mixed-steps"] == "two" and modes["constant-pairs"] == "two" and modes["sorted-pairs"] == "two"
    # the mixed block has tiles for both scatter kernels (k_ib_hist: at most 48 distinct bytes)
    L = ic.mixed_L()
    kinds = {np.unique(L[o:o + 4096]).size <= 48 for o in range(0, L.size, 4096)}
    assert kinds == {True, False}


@pytest.mark.skipif(not have_ref(), reason="reference build (oracle/_ref) not present")
def test_oracle_inverse_vs_reference(orc):
    """Oracle.bwt_decode against the reference's bra_bwt_decode2 on arbitrary (L, pi)."""
    ref = Reference()
    n = 0
    for name, L, p in ic.single_cases():
        if L.size <= ic.SMALL:
            assert orc.bwt_decode(L.tobytes(), p) == ref.bwt_decode(L.tobytes(), p), name
            n += 1
    assert n > 250
