"""Inputs of the inverse-BWT tests (test_ibwt_cases.py on the CPU, test_gpu_ibwt.py on the GPU): byte
strings L with a primary index that are NOT outputs of a forward BWT -- the reference's
bra_bwt_decode2 is defined for any of them -- and a helper that wraps blocks of them into what
BlockCodec.decode takes.  Every expected output is the oracle's; scripts/ibwt_hops.py says which
kernel paths an input reaches.  Not a test module."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = 268


def _load_model():
    spec = importlib.util.spec_from_file_location("ibwt_hops", os.path.join(ROOT, "scripts", "ibwt_hops.py"))
    mod = importlib.util.module_from_spec(spec)
    import sys

    sys.modules.setdefault("ibwt_hops", mod)  # dataclasses looks the defining module up by name
    spec.loader.exec_module(mod)
    return mod


model = _load_model()

ALPHABETS = (2, 4, 16, 256)
# 1, 2; around the 16-byte flush and the 64-position ballot round; around the 4096-byte tile; one and
# several tiles with a ragged end; the last n with S = 64 (16384 splitters), the first with S = 128
# (the two-step walk), and S = 512
SIZES = (1, 2, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 65536, 100003, 1 << 20, (1 << 20) + 1, (1 << 22) + 5)
SMALL = 100003  # up to here every alphabet meets every primary index; above, see random_cases
MIXED_N = 200000
TRANSFORM_MAX = 1 << 21


def random_L(seed: int, n: int, alphabet: int) -> np.ndarray:
    return np.random.default_rng([seed, n, alphabet]).integers(0, alphabet, n, dtype=np.uint8)


def mixed_L(n: int = MIXED_N) -> np.ndarray:
    """16 symbols, then uniform bytes: k_ib_hist hands the tiles of the first half to k_ib_scatter2
    and those of the second to k_ib_scatter3."""
    return np.concatenate([random_L(5, n // 2, 16) + 97, random_L(6, n - n // 2, 256)])


def constant_L(n: int, v: int = 0x41) -> np.ndarray:
    return np.full(n, v, np.uint8)


def sorted_L(n: int) -> np.ndarray:
    """Sorted, 16 symbols (frequent enough that the block suits the two-step walk)."""
    return np.sort(random_L(7, n, 16))


def primary_indices(n: int, seed: int = 0):
    """0, n-1, one before / on / after the first splitter, the last regular splitter and the
    position after it (the last partial stride), and one drawn position -- those below n."""
    shift, ns = model.geometry(n)
    S = 1 << shift
    drawn = int(np.random.default_rng([seed, n]).integers(0, n))
    out = []
    for p in (0, n - 1, S - 1, S, S + 1, (ns - 1) * S, (ns - 1) * S + 1, drawn):
        if 0 <= p < n and p not in out:
            out.append(p)
    return out


def random_cases(n: int):
    """[(name, L, pi)] for one size.  Up to SMALL every alphabet meets every primary index; above
    that the primary indices are dealt round robin over the alphabets, so each of them and each
    alphabet still occurs at every size while a size stays a few seconds of oracle time."""
    pis = primary_indices(n)
    out = []
    for ai, a in enumerate(ALPHABETS):
        L = random_L(1, n, a)
        for i, p in enumerate(pis):
            if n <= SMALL or i % len(ALPHABETS) == ai:
                out.append((f"random{a}-n{n}-pi{p}", L, p))
    return out


def mixed_cases():
    L = mixed_L()
    return [(f"mixed-n{L.size}-pi{p}", L, p) for p in primary_indices(L.size)[:4]]


def identity_cases():
    """T is the identity: every hop is one byte, the output is n copies of L[pi].  2^20 + 1 walks
    two steps per load, where a hop ends at the intermediate index."""
    out = []
    for n in (65536, (1 << 20) + 1):
        S = 1 << model.geometry(n)[0]
        for kind, L in (("constant", constant_L(n)), ("sorted", sorted_L(n))):
            for p in (3 * S, 3 * S + 1, n - 1):
                out.append((f"{kind}-n{n}-pi{p}", L, p))
    return out


# (n, a, pi): T(y) = y + a mod n.  A cycle of 7; a = 2: the odd positions hold no regular splitter,
# so an odd pi walks n / 2 bytes in one hop -- a long overflow chain at 65536, more chunks than the
# pool holds at 2^21 -- and an even pi walks regular strides; a coprime to n: one cycle of n.
ROTATIONS = ((70000, 10000, 3), (65536, 2, 12345), (65536, 2, 12344), (1 << 21, 2, 12345), (1 << 21, 2, 12344), (65536, 4099, 77))
EXHAUSTING = (1 << 21, 2, 12345)


def rotation_cases():
    return [(f"rotation-n{n}-a{a}-pi{p}", model.rotation(n, a), p) for n, a, p in ROTATIONS]


def single_cases():
    out = []
    for n in SIZES:
        out += random_cases(n)
    return out + mixed_cases() + identity_cases() + rotation_cases()


# ---- batches ---------------------------------------------------------------------------------------
def batch_cases():
    """{name: [(L, pi)]}: equal-size blocks, the last one ragged."""
    out = {}
    n = 65536
    out["nine-64k"] = [(random_L(20 + b, n, ALPHABETS[b % 4]), int(p)) for b, p in
                       enumerate([0, n - 1, 63, 64, 65, 65472, 65473, 31337, 4096])]
    n = (1 << 20) + 1
    sym16 = [(random_L(30, n, 16), 127), (random_L(31, n, 16), 128), (random_L(32, 50001, 16), 50000)]
    out["two-step"] = sym16
    out["one-step-if"] = [sym16[0], (random_L(33, n, 256), 129), sym16[2]]
    n = 1 << 21
    out["mixed-steps"] = [(random_L(40, n, 16), n - 1), (random_L(41, n, 4), 128), (random_L(42, 100003, 16), 99968)]
    # one block each, so that the diagnostics speak of that block alone
    out["rotation-64k-odd"] = [(model.rotation(65536, 2), 12345)]
    out["rotation-cycle-7"] = [(model.rotation(70000, 10000), 3)]
    out["constant-pairs"] = [(constant_L((1 << 20) + 1), 385)]
    out["sorted-pairs"] = [(sorted_L((1 << 20) + 1), 384)]
    return out


def exhausting_batch():
    """The rotation by 2 with an odd primary index between two ordinary blocks.  The block size is
    the smallest at which three blocks' pool (a fresh context's) cannot hold the long hop: the hop
    needs about n / 512 chunks, the pool has about 0.14 chunks per splitter, so S must exceed
    72 x blocks, and 2^21 + 2 is the first even size with S = 256."""
    n = (1 << 21) + 2
    return [(random_L(50, n, 16), 5), (model.rotation(n, 2), 12345), (random_L(51, n, 16), n - 1)]


def words_batch(orc, blocks: int = 5, n: int = 65536):
    """An ordinary valid batch: (data, [(L, pi)]) of forward BWTs (the oracle's) of text blocks."""
    from files_cases import words

    rng = np.random.default_rng(60)
    data = words(rng, blocks * n - 1234)
    out = []
    for o in range(0, len(data), n):
        L, pi = orc.bwt_encode(data[o:o + n])
        out.append((np.frombuffer(L, np.uint8), pi))
    return data, out


def encode_batch(orc, blocks):
    """What BlockCodec.decode takes for blocks [(L, pi)] whose inverse BWT input is exactly L:
    (headers [nb, 268] u8, offsets [nb + 1] i64, payload u8, total, block_size), each block's L run
    through the oracle's MTF, RLE and Huffman encoders and given the in-memory chunk header
    (pi, 256 code lengths, orig_size, encoded_size, little-endian)."""
    bs = int(blocks[0][0].size)
    assert all(L.size == bs for L, _ in blocks[:-1]) and 0 < blocks[-1][0].size <= bs
    hdr = np.zeros((len(blocks), HDR), np.uint8)
    off = np.zeros(len(blocks) + 1, np.int64)
    pays = []
    for b, (L, pi) in enumerate(blocks):
        assert 0 <= pi < L.size
        lens, osz, esz, pay = orc.huffman_encode(orc.rle_encode(orc.mtf_encode(L.tobytes())))
        assert len(lens) == 256 and len(pay) == esz
        h = int(pi).to_bytes(4, "little") + lens + int(osz).to_bytes(4, "little") + int(esz).to_bytes(4, "little")
        hdr[b] = np.frombuffer(h, np.uint8)
        off[b + 1] = off[b] + esz
        pays.append(np.frombuffer(pay, np.uint8))
    payload = np.concatenate(pays + [np.zeros(16, np.uint8)])
    return hdr, off, payload, sum(int(L.size) for L, _ in blocks), bs


def expected(orc, blocks) -> np.ndarray:
    return np.frombuffer(b"".join(orc.bwt_decode(L.tobytes(), int(pi)) for L, pi in blocks), np.uint8)


def predict(blocks, pool_cap=None):
    """What bra_gpu_debug_ibwt_path must report for a batch: dict(walk, chunks, nsplit, fresh_cap);
    with the context's pool_cap also path ("main" or "fallback")."""
    hs = [model.hops(L, int(pi)) for L, pi in blocks]
    nsplit = sum(h.nsplit for h in hs)
    out = dict(walk=model.walk_mode(hs), chunks=sum(h.chunks for h in hs), nsplit=nsplit, fresh_cap=model.pool_capacity(nsplit))
    if pool_cap is not None:
        out["path"] = "fallback" if out["chunks"] > pool_cap else "main"
    return out
