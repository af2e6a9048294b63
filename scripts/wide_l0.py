"""Host emulation of a wide first BWT split (bwt.hip level 0 placing every rotation by its first two
packed key bytes instead of one) on one synthetic block: bits per character, the number B of
non-empty 16-bit packed prefixes, how long the runs are that one tile writes into one prefix's
sub-bucket (the unit a staged scatter can store coalesced) for tiles of 4 Ki / 8 Ki / 16 Ki / 32 Ki
positions, and what the elements become at depth 2.  Measurement / design aid only (CPU, numpy).

    python scripts/wide_l0.py [kind] [block_size]        kind: text | sym16 | random | tiled
    python scripts/wide_l0.py --table                    the DESIGN table (markdown)

`prefix16` and `prefix_count` are also what tests use to build inputs with a known B.
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TILES = (4096, 8192, 16384, 32768)
JOB_WAVE, JOB_WG = 256, 1024  # bwt.hip: JOB_MAX, the largest workgroup job


def pack_bits(blk: np.ndarray):
    """(codes, b): alphabet ranks of the block's bytes and the bits per character k_pack uses."""
    vals = np.unique(blk)
    b = 1 if vals.size <= 2 else int(vals.size - 1).bit_length()
    rank = np.zeros(256, np.int64)
    rank[vals] = np.arange(vals.size)
    return rank[blk], b


def prefix16(blk: np.ndarray) -> np.ndarray:
    """Key bytes 0 and 1 of every rotation of the block's packed cyclic string (pk_bitpos semantics:
    rotation i starts at bit i * b, the string continues cyclically past its last bit)."""
    codes, b = pack_bits(np.asarray(blk, np.uint8))
    k = -(-16 // b)  # characters that cover 16 bits
    v = np.zeros(codes.size, np.int64)
    for j in range(k):
        v = (v << b) | np.roll(codes, -j)
    return (v >> (k * b - 16)).astype(np.uint16)


def prefix_count(blk: np.ndarray) -> int:
    """B: the number of distinct 16-bit packed prefixes among the block's rotations."""
    return int(np.unique(prefix16(blk)).size)


def run_stats(pfx: np.ndarray, tile: int):
    """Lengths of the (tile, prefix) runs: what one tile stores contiguously into one sub-bucket."""
    key = (np.arange(pfx.size, dtype=np.int64) // tile) << 16 | pfx
    return np.unique(key, return_counts=True)[1]


def depth2_classes(pfx: np.ndarray):
    """Element counts per class after the wide split.  A first-byte bucket of <= 1024 elements is a
    job at depth 1 (one dense bin for the whole d0); the others split by the 16-bit prefix."""
    c0 = np.bincount(pfx >> 8, minlength=256)
    small0 = c0 <= JOB_WG
    c16 = np.bincount(pfx, minlength=65536)
    c16 = np.where(np.repeat(small0, 256), 0, c16)
    out = {
        "depth1_jobs": int(c0[small0].sum()),
        "single": int(c16[c16 == 1].sum()),
        "wave_jobs": int(c16[(c16 > 1) & (c16 <= JOB_WAVE)].sum()),
        "wg_jobs": int(c16[(c16 > JOB_WAVE) & (c16 <= JOB_WG)].sum()),
        "continue": int(c16[c16 > JOB_WG].sum()),
        "continue_buckets": int((c16 > JOB_WG).sum()),
    }
    # dense bins the device would use: one per non-empty prefix of a big d0, one per small non-empty d0
    out["dense_bins"] = int((c16 > 0).sum() + (small0 & (c0 > 0)).sum())
    return out


def make_block(kind: str, bs: int) -> np.ndarray:
    sys.path.insert(0, ROOT)
    bra = importlib.import_module("br-archive_amd")
    kid = {"text": bra.SYNTH_TEXT, "random": bra.SYNTH_RANDOM, "sym16": bra.SYNTH_SYM16, "tiled": bra.SYNTH_TILED}[kind]
    return bra.synth_fill(kid, bs, bs)


def stats(kind: str, bs: int):
    blk = make_block(kind, bs)
    _, b = pack_bits(blk)
    pfx = prefix16(blk)
    res = {"kind": kind, "block": bs, "bits": b, "B": int(np.unique(pfx).size), "tiles": {}, "classes": depth2_classes(pfx)}
    for t in TILES:
        if t > bs:
            continue
        r = run_stats(pfx, t)
        el = lambda lo, hi=1 << 30: float(r[(r >= lo) & (r < hi)].sum()) / bs  # noqa: E731
        res["tiles"][t] = {"mean": float(bs) / r.size, "ge8": el(8), "ge16": el(16),
                           "hist": [el(1, 2), el(2, 4), el(4, 8), el(8, 16), el(16, 32), el(32, 64), el(64)]}
    return res


def show(res):
    c = res["classes"]
    print(f"{res['kind']} block {res['block']}: {res['bits']} bits/char, B = {res['B']} non-empty 16-bit prefixes "
          f"({c['dense_bins']} dense bins with small first-byte buckets merged)")
    print(f"  depth 2: continue {c['continue']} in {c['continue_buckets']} buckets, workgroup jobs {c['wg_jobs']}, wave jobs {c['wave_jobs']}, "
          f"single {c['single']}, depth-1 jobs {c['depth1_jobs']}")
    print("  elements by (tile, prefix) run length:   mean   >=8  >=16 |     1   2-3   4-7  8-15 16-31 32-63  64+")
    for t, s in res["tiles"].items():
        print(f"  tile {t:6d}: {s['mean']:27.1f} {s['ge8']:5.2f} {s['ge16']:5.2f} | " + " ".join(f"{x:5.2f}" for x in s["hist"]))


TABLE = (("text", 1 << 20), ("sym16", 1 << 20), ("sym16", 8 << 20), ("random", 1 << 20), ("tiled", 1 << 16))


def table():
    print("| input | bits/char | B | mean run, elements in runs ≥ 16 / ≥ 8 at tile 4 Ki | 8 Ki | 16 Ki | 32 Ki | continue past depth 2 (buckets) | job-bound |")
    print("|---|---|---|---|---|---|---|---|---|")
    for kind, bs in TABLE:
        r = stats(kind, bs)
        c = r["classes"]
        cells = [(f"{s['mean']:.1f}, {s['ge16']:.2f} / {s['ge8']:.2f}" if s else "–") for s in (r["tiles"].get(t) for t in TILES)]
        name = f"{kind} {bs >> 20} MiB" if bs >= 1 << 20 else f"{kind} {bs >> 10} KiB"
        print(f"| {name} | {r['bits']} | {r['B']} | " + " | ".join(cells) +
              f" | {c['continue']} ({c['continue_buckets']}) | {r['block'] - c['continue']} |")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--table":
        table()
    else:
        show(stats(sys.argv[1] if len(sys.argv) > 1 else "text", int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 20))
