"""The inverse BWT (csrc/ibwt.hip) on inputs that are not outputs of a forward BWT.

The reference's bra_bwt_decode2 is defined for any byte string L and any primary index below its
length, and a damaged but well-formed archive hands the kernels exactly that.  Checker: the
oracle's inverse (oracle/bra_oracle.c, pinned to the reference on these inputs by
test_ibwt_cases.py), bit for bit.  Which kernel paths a case reaches is the claim of the host model
(scripts/ibwt_hops.py, asserted in test_ibwt_cases.py); after every batched decode
bra_gpu_debug_ibwt_path must report the path, the walk mode and the overflow chunks the model
predicts, so that no case passes by having taken another path.
"""
import importlib

import numpy as np
import pytest

import ibwt_cases as ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bra():
    return importlib.import_module("br-archive_amd")


@pytest.fixture(scope="module")
def codec(bra):
    c = bra.BlockCodec(0)
    yield c
    c.close()


def _same(got: bytes, want: bytes, what: str):
    if got != want:
        g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        assert g.size == w.size, f"{what}: {g.size} bytes, expected {w.size}"
        bad = np.flatnonzero(g != w)
        raise AssertionError(f"{what}: {bad.size} of {w.size} bytes differ, first at {bad[:6].tolist()}, last at {int(bad[-1])}")


def _check_singles(bra, orc, cases):
    for name, L, p in cases:
        _same(bra.bwt_decode(L.tobytes(), p), orc.bwt_decode(L.tobytes(), p), name)


# ---- single blocks through bra_bwt_decode2 -------------------------------------------------------------
@pytest.mark.parametrize("n", ic.SIZES)
def test_random_blocks(bra, orc, n):
    """Uniform L over 2, 4, 16 and 256 symbols with the primary index at every position relative to
    the splitters: partial cycles, hops of every length mod 16, hops into the overflow pool."""
    _check_singles(bra, orc, ic.random_cases(n))


def test_block_for_both_scatter_kernels(bra, orc):
    _check_singles(bra, orc, ic.mixed_cases())


def test_identity_transform(bra, orc):
    """Constant and sorted L: every hop is one byte and the output is n copies of L[pi]."""
    for name, L, p in ic.identity_cases():
        want = bytes([int(L[p])]) * L.size
        assert orc.bwt_decode(L.tobytes(), p) == want, name
        _same(bra.bwt_decode(L.tobytes(), p), want, name)


def test_rotations(bra, orc):
    """T(y) = y + a mod n: a cycle of 7, one hop of n / 2 bytes (with and without enough overflow
    chunks: at 2^21 the pool of the library's own context runs out unless earlier calls grew it), regular
    strides, one cycle of n."""
    _check_singles(bra, orc, ic.rotation_cases())


@pytest.mark.parametrize("group", [n for n in ic.SIZES if n <= ic.TRANSFORM_MAX] + ["special"])
def test_transform_requested(bra, orc, group):
    """bra_bwt_decode2 with a transform buffer, as the shipped front end calls it for every chunk:
    the two-walk path, on every single-block case up to 2^21 bytes.  The transform is the
    reference's (the stable sort of the positions by byte) and the output the oracle's."""
    if group == "special":
        cases = [c for c in ic.mixed_cases() + ic.identity_cases() + ic.rotation_cases() if c[1].size <= ic.TRANSFORM_MAX]
        assert len(cases) == 4 + 12 + len(ic.ROTATIONS)
    else:
        cases = ic.random_cases(group)
    for name, L, p in cases:
        out, T = bra.bwt_decode(L.tobytes(), p, want_transform=True)
        assert T.dtype == np.uint32 and T.size == L.size
        assert np.array_equal(T, np.argsort(L, kind="stable")), f"{name}: transform"
        _same(out, orc.bwt_decode(L.tobytes(), p), name)


# ---- batches through bra_gpu_decode_blocks -------------------------------------------------------------
def _decode(codec, enc):
    import torch

    hdr, off, pay, total, bs = enc
    out = codec.decode(torch.from_numpy(hdr).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(pay).cuda(), total, bs)
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes(), codec.debug_ibwt_path()


def _check_batch(codec, orc, blocks, what):
    """Decode, compare with the oracle, and hold the diagnostics against the model."""
    got, info = _decode(codec, ic.encode_batch(orc, blocks))
    pred = ic.predict(blocks, info["pool_cap"])
    print(what, info, pred)
    assert info["path"] == pred["path"], (what, info, pred)
    assert info["walk"] == pred["walk"], (what, info, pred)
    assert info["pool_used"] == pred["chunks"], (what, info, pred)  # the walk counts on past the capacity
    _same(got, ic.expected(orc, blocks).tobytes(), what)
    return info, pred


@pytest.mark.parametrize("name", sorted(ic.batch_cases()))
def test_batches(codec, orc, name):
    """Nine 64 KiB blocks (one step per load); blocks of 2^20 + 1 over 16 symbols (two steps), the
    same with a uniform block among them (one step for the whole batch); 2^21 with a ragged 100 KB
    block (S = 128 and S = 64 in one call); and single special blocks whose chunk count and walk
    mode the diagnostics must show."""
    info, pred = _check_batch(codec, orc, ic.batch_cases()[name], name)
    assert info["path"] == "main" and pred["chunks"] <= info["pool_cap"]


def test_pool_exhaustion_and_the_decode_after_it(bra, orc):
    """A hop longer than the overflow pool of a fresh context, between two ordinary blocks: the walk
    runs out of chunks, the two-walk path redoes the batch, and the output is the oracle's.  Then an
    ordinary valid batch on the same context is still exact (nothing stale from the exhausted call:
    hop_ovf, ovl_next, cyc)."""
    blocks = ic.exhausting_batch()
    c = bra.BlockCodec(0)
    try:
        assert c.debug_ibwt_path()["path"] == "none"
        info, pred = _check_batch(c, orc, blocks, "exhausting batch")
        assert info["pool_cap"] == pred["fresh_cap"]  # a new context: not what ran before
        assert pred["chunks"] > info["pool_cap"]
        assert info["path"] == "fallback" and info["pool_used"] > info["pool_cap"] and info["walk"] == "two"
        data, valid = ic.words_batch(orc)
        got, after = _decode(c, ic.encode_batch(orc, valid))
        _same(got, data, "valid batch after the exhausted one")
        assert ic.expected(orc, valid).tobytes() == data
        p2 = ic.predict(valid, after["pool_cap"])
        assert (after["path"], after["walk"], after["pool_used"]) == ("main", "one", p2["chunks"]), (after, p2)
    finally:
        c.close()
