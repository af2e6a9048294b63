"""The wide first BWT split (csrc/bwt.hip, k_l0w_*): rotations placed by their first two packed key
bytes in one pass when every block of the call has between 2 and 8192 distinct 16-bit packed
prefixes and at least one tile of 16384 positions; otherwise the 8-bit level 0.

Checker: oracle.Oracle().encode_block per block (primary index, code lengths, sizes, payload), bit
exact.  Every case also asserts the path the codec reports for the call (BlockCodec.debug_bwt_path),
so no case passes by taking the other path; the prefix counts come from scripts/wide_l0.py (CPU).
"""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import wide_l0  # noqa: E402

TILE, MAX_BINS = 16384, 8192
WIDE, NARROW = 1, 0


@pytest.fixture(scope="module")
def bra():
    return importlib.import_module("br-archive_amd")


@pytest.fixture(scope="module")
def codec(bra):
    c = bra.BlockCodec(0)
    yield c
    c.close()


def _encode(codec, data, bs):
    import torch

    hdr, off, pay = codec.encode(torch.from_numpy(data).cuda(), bs)
    torch.cuda.synchronize()
    return hdr.cpu().numpy(), off.cpu().numpy(), pay.cpu().numpy()


def _check(bra, codec, orc, data, bs, path, bins=None, expect=None):
    """Encode data in blocks of bs; every block against the oracle (or expect[b]: a golden entry)."""
    hdr, off, pay = _encode(codec, data, bs)
    got_path, got_bins = codec.debug_bwt_path()
    assert got_path == path, f"path {got_path} (max prefixes {got_bins}), expected {path}"
    if bins is not None:
        assert got_bins == bins
    for b in range(codec.num_blocks(data.size, bs)):
        blk = data[b * bs:(b + 1) * bs].tobytes()
        if expect is not None:
            g = expect[b]
            want = (g["pi"], g["lengths"], g["orig_size"], g["encoded_size"], g["payload"])
        else:
            ch = orc.encode_block(blk)
            want = (ch.primary_index, ch.lengths, ch.orig_size, ch.encoded_size, ch.payload)
        pi, lens, osz, esz = bra.parse_header(hdr[b].tobytes())
        assert (pi, lens, osz, esz) == want[:4], f"block {b}: header"
        assert int(off[b + 1] - off[b]) == esz and pay[off[b]: off[b] + esz].tobytes() == want[4], f"block {b}: payload"
    return hdr, off, pay


CHILD = """
import importlib, sys
import numpy as np, torch
sys.path.insert(0, {root!r})
bra = importlib.import_module("br-archive_amd")
data = bra.synth_fill({kind}, {total}, {bs})
c = bra.BlockCodec(0)
hdr, off, pay = c.encode(torch.from_numpy(data).cuda(), {bs})
torch.cuda.synchronize()
assert c.debug_bwt_path()[0] == 0, c.debug_bwt_path()
np.savez({out!r}, hdr=hdr.cpu().numpy(), off=off.cpu().numpy(), pay=pay[: int(off[-1].item())].cpu().numpy())
"""


@pytest.mark.parametrize("kind", ["text", "sym16"])
def test_wide_matches_oracle_and_narrow(bra, codec, orc, tmp_path, kind):
    """3 blocks of 64 KiB: the wide path, and byte-identical to the same call with BRA_L0_WIDE=0 (read
    when a context is created, so in a fresh process)."""
    kid = {"text": bra.SYNTH_TEXT, "sym16": bra.SYNTH_SYM16}[kind]
    bs, total = 65536, 3 * 65536
    data = bra.synth_fill(kid, total, bs)
    bins = max(wide_l0.prefix_count(data[k * bs:(k + 1) * bs]) for k in range(3))
    hdr, off, pay = _check(bra, codec, orc, data, bs, WIDE, bins)
    out = str(tmp_path / "narrow.npz")
    env = dict(os.environ, BRA_L0_WIDE="0")
    subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) +
                   ["-c", CHILD.format(root=ROOT, kind=kid, total=total, bs=bs, out=out)], check=True, env=env, timeout=300)
    z = np.load(out)
    assert np.array_equal(z["hdr"], hdr) and np.array_equal(z["off"], off) and np.array_equal(z["pay"], pay[: int(off[-1])])


@pytest.mark.parametrize("n", [TILE, TILE + 1, 3 * TILE - 1])
def test_lengths_around_the_tile(bra, codec, orc, n):
    data = bra.synth_fill(bra.SYNTH_TEXT, 4 * TILE, 4 * TILE)[:n].copy()
    _check(bra, codec, orc, data, n, WIDE, wide_l0.prefix_count(data))


def test_short_last_block_takes_the_narrow_path(bra, codec, orc):
    bs = 2 * TILE
    data = bra.synth_fill(bra.SYNTH_TEXT, 2 * bs + 1000, bs)
    _check(bra, codec, orc, data, bs, NARROW)


def _block_with_pairs(target: int, n: int, seed: int) -> np.ndarray:
    """n bytes over all 256 byte values (8 bits per character: the 16-bit prefix is a byte pair) whose
    set of adjacent pairs has `target` members before the cyclic wrap adds its own: a ramp 0..255,
    random bytes until the set is full, then a walk along pairs already seen."""
    rng = np.random.default_rng(seed)
    s = list(range(256))
    succ = {i: [i + 1] for i in range(255)}
    pairs = {(i, i + 1) for i in range(255)}
    while len(s) < n:
        y = s[-1]
        if len(pairs) < target:
            x = int(rng.integers(0, 256))
            if (y, x) not in pairs:
                pairs.add((y, x))
                succ.setdefault(y, []).append(x)
        else:
            x = succ[y][int(rng.integers(0, len(succ[y])))]
        s.append(x)
    return np.array(s, np.uint8)


def test_max_bins_boundary(bra, codec, orc):
    """B at / just below the limit takes the wide path, just above the narrow one; the reported B is
    the CPU count (the wrap pair included)."""
    below = _block_with_pairs(MAX_BINS - 1, 20000, 1)
    above = _block_with_pairs(MAX_BINS + 1, 20000, 2)
    b_lo, b_hi = wide_l0.prefix_count(below), wide_l0.prefix_count(above)
    assert b_lo in (MAX_BINS - 1, MAX_BINS) and b_hi in (MAX_BINS + 1, MAX_BINS + 2)
    _check(bra, codec, orc, below, below.size, WIDE, b_lo)
    _check(bra, codec, orc, above, above.size, NARROW, b_hi)


def test_mixed_batch_with_a_random_block_is_narrow(bra, codec, orc):
    bs = 65536
    data = np.concatenate([bra.synth_fill(bra.SYNTH_TEXT, 2 * bs, bs), bra.synth_fill(bra.SYNTH_RANDOM, bs, bs)])
    assert wide_l0.prefix_count(data[2 * bs:]) > MAX_BINS
    _check(bra, codec, orc, data, bs, NARROW)
    assert codec.debug_bwt_path()[1] > MAX_BINS  # (a lower bound: a tile that alone exceeds the limit gives its block up)


def test_tiled_block_ends_in_the_fallback(bra, codec, golden):
    """test.txt tiled to 64 KiB: 22 prefixes, every rotation tied to the depth cap (prefix doubling)."""
    g = golden["cfg1_tiled_65536"]
    data = np.frombuffer(g["input"], np.uint8).copy()
    _check(bra, codec, None, data, 65536, WIDE, wide_l0.prefix_count(data), expect=[g])


def test_two_symbols_alternating(bra, codec, orc):
    data = np.tile(np.frombuffer(b"ab", np.uint8), TILE // 2 + 3)
    assert wide_l0.prefix_count(data) == 2
    _check(bra, codec, orc, data, data.size, WIDE, 2)


def test_one_symbol_is_narrow(bra, codec, orc):
    data = np.full(TILE, 0x41, np.uint8)
    _check(bra, codec, orc, data, data.size, NARROW, 1)


def test_cyclic_wrap_prefix(bra, codec, orc):
    """'z' occurs only in the block's last two and first two bytes, so the prefixes of the rotations
    that start in the last three bytes exist only across the wrap."""
    rng = np.random.default_rng(5)
    data = np.frombuffer(b"abcdefgh", np.uint8)[rng.integers(0, 8, 20000)].copy()  # 9 symbols, 4 bits: a prefix is 4 characters
    data[:2] = data[-2:] = ord("z")
    pf = wide_l0.prefix16(data)
    bins = int(np.unique(pf).size)
    assert bins <= MAX_BINS and all(np.count_nonzero(pf == pf[i]) == 1 for i in (data.size - 3, data.size - 2, data.size - 1))
    _check(bra, codec, orc, data, data.size, WIDE, bins)


def test_one_prefix_holds_most_of_the_block(bra, codec, orc):
    """Runs of 40 'a' closed by a random letter: the prefix 'aaa' + a zero bit holds ~90 % of 64 KiB,
    several tiles' worth, so single runs span the whole staging of a tile."""
    rng = np.random.default_rng(6)
    units = np.full((65536 // 41 + 1, 41), ord("a"), np.uint8)
    units[:, 40] = np.frombuffer(b"bcdefghijklmnopqrstuvwxyz", np.uint8)[rng.integers(0, 25, units.shape[0])]
    data = units.ravel()[:65536].copy()
    pf = wide_l0.prefix16(data)
    assert np.bincount(pf).max() > 32768
    _check(bra, codec, orc, data, data.size, WIDE, int(np.unique(pf).size))


def test_block_of_128_tiles(bra, codec, orc):
    """One 2 MiB block of 16-symbol data: more than 64 wide tiles in one block."""
    data = bra.synth_fill(bra.SYNTH_SYM16, 2 << 20, 2 << 20)
    _check(bra, codec, orc, data, data.size, WIDE, wide_l0.prefix_count(data))
