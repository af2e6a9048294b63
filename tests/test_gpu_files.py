"""Many files in one device call (include/bra_hip_files.h: bra_gpu_compress_files /
bra_gpu_decompress_files) against the oracle's compress loop run file by file: stream bytes, sizes,
chunk counts, store-or-compress verdicts and both CRC32C values per file, bit for bit.  Expected
values never come from the library under test.
"""
import importlib

import numpy as np
import pytest

import files_cases as fc

pytestmark = pytest.mark.gpu

CS = fc.CS


@pytest.fixture(scope="module")
def bra():
    return importlib.import_module("br-archive_amd")


@pytest.fixture(scope="module")
def codec(bra):
    c = bra.BlockCodec(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def size_list(orc):
    files = fc.size_list_files()
    return files, fc.expected(orc, files, CS)


@pytest.fixture(scope="module")
def small_block(orc):
    files = fc.small_block_files()
    return files, fc.expected(orc, files, 4096)


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(out, res, files, exp):
    """One compress_files result against the oracle, file by file."""
    out_h = out.cpu().numpy()
    assert len(res) == len(files)
    pos = 0
    for f, (r, e) in enumerate(zip(res, exp)):
        assert int(r["off"]) == pos, f  # contiguous, in file order
        assert int(r["size"]) == len(e["stream"]), (f, len(files[f]))
        assert out_h[pos:pos + len(e["stream"])].tobytes() == e["stream"], (f, len(files[f]))
        assert int(r["num_chunks"]) == e["num_chunks"], f
        assert int(r["compressed"]) == e["compressed"], (f, len(files[f]))
        assert int(r["chunks_crc"]) == e["chunks_crc"], (f, len(files[f]))
        assert int(r["raw_crc"]) == e["raw_crc"], (f, len(files[f]))
        pos += len(e["stream"])
    assert pos == out_h.size == int(res["size"].sum())


def test_size_list_generator_covers_both_verdicts(size_list):
    """What the oracle says about the test's own inputs (no GPU work): both verdicts and the chunk
    counts 1, 2 and 3 occur, so the comparisons below see every case."""
    files, exp = size_list
    verdicts = [e["compressed"] for e in exp]
    assert verdicts.count(0) >= 2 and verdicts.count(1) >= 2
    assert {1, 2, 3} <= {e["num_chunks"] for e in exp}
    by_len = {len(f): e for f, e in zip(files, exp)}
    assert by_len[262145]["num_chunks"] == 2 and by_len[524295]["num_chunks"] == 3
    assert by_len[1]["compressed"] == 0 and by_len[4096]["compressed"] == 0 and by_len[524288]["compressed"] == 1


@pytest.mark.parametrize("layout", ["packed", "aligned16"])
def test_size_list_at_256k(codec, size_list, layout):
    """1 byte next to 512 KiB + 7 in one call, back to back from an odd offset or every file at a
    16-byte-aligned offset with gaps."""
    files, exp = size_list
    buf, offs, lens = fc.pack(files, lead=3) if layout == "packed" else fc.pack(files, align=16)
    assert layout == "aligned16" or any(o % 2 for o in offs)
    out, res = codec.compress_files(_cuda(buf), offs, lens, CS)
    _check(out, res, files, exp)


def test_small_block_size(codec, small_block):
    files, exp = small_block
    assert sum(1 for f in files if not f) == 2 and max(e["num_chunks"] for e in exp) >= 4
    buf, offs, lens = fc.pack(files, lead=1)
    out, res = codec.compress_files(_cuda(buf), offs, lens, 4096)
    _check(out, res, files, exp)
    for r, f in zip(res, files):
        if not f:
            assert (int(r["size"]), int(r["num_chunks"]), int(r["compressed"]), int(r["chunks_crc"]), int(r["raw_crc"])) == (0, 0, 0, 0, 0)


def test_many_files_round_trip(codec, orc):
    """8192 files of 1..2048 bytes in one compress call, the compressed ones back in one decompress
    call (a capacity layout of the decode would need 8192 x 256 KiB = 2 GiB)."""
    import torch

    rng = np.random.default_rng(8192)
    n = 8192
    lens = [int(x) for x in rng.integers(1, 2049, n)]
    pool = np.frombuffer(fc.words(rng, 2 << 20), np.uint8)
    files = []
    for i, ln in enumerate(lens):
        if i % 3 == 2:
            files.append(rng.integers(0, 256, ln, dtype=np.uint8).tobytes())
        else:
            st = int(rng.integers(0, pool.size - ln))
            files.append(pool[st:st + ln].tobytes())
    buf, offs, _ = fc.pack(files)
    d = _cuda(buf)
    out, res = codec.compress_files(d, offs, lens, CS)
    assert int(res["size"].sum()) == out.numel()
    assert np.array_equal(res["off"], np.concatenate([[0], np.cumsum(res["size"])[:-1]]))
    assert (res["num_chunks"] == 1).all()
    assert np.array_equal(res["compressed"], (res["size"] < np.array(lens, np.uint64)).astype(np.uint32))
    sel = np.flatnonzero(res["compressed"] == 1)
    assert 1000 < sel.size < n  # words compress, random bytes do not
    # 64 sampled files against the oracle
    out_h = out.cpu().numpy()
    for f in rng.choice(n, 64, replace=False):
        stream, crc, _ = orc.compress_chunks(files[f], CS)
        r = res[f]
        assert out_h[int(r["off"]):int(r["off"] + r["size"])].tobytes() == stream, f
        assert (int(r["chunks_crc"]), int(r["raw_crc"])) == (crc, orc.crc32c(files[f])), f
    # the round trip of every compressed file
    dec, dres = codec.decompress_files(out, [int(x) for x in res["off"][sel]], [int(x) for x in res["size"][sel]], CS)
    want = np.concatenate([np.frombuffer(files[f], np.uint8) for f in sel])
    assert dec.numel() == want.size and torch.equal(dec, _cuda(want))
    sl = np.array([lens[f] for f in sel], np.uint64)
    assert np.array_equal(dres["size"], sl)
    assert np.array_equal(dres["off"], np.concatenate([[0], np.cumsum(sl)[:-1]]).astype(np.uint64))
    assert np.array_equal(dres["chunks_crc"], res["chunks_crc"][sel])
    assert np.array_equal(dres["raw_crc"], res["raw_crc"][sel])
    assert (dres["num_chunks"] == 1).all() and (dres["compressed"] == 1).all()


def test_multi_chunk_decode(codec, size_list, small_block):
    """The decode side over files of 1, 2 and 3 chunks and ragged tails, at both block sizes."""
    import torch

    for (files, exp), bs in ((size_list, CS), (small_block, 4096)):
        keep = [i for i, e in enumerate(exp) if e["compressed"]]
        streams = np.concatenate([np.frombuffer(exp[i]["stream"], np.uint8) for i in keep])
        sizes = [len(exp[i]["stream"]) for i in keep]
        offs = [int(x) for x in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
        dec, dres = codec.decompress_files(_cuda(streams), offs, sizes, bs)
        want = np.concatenate([np.frombuffer(files[i], np.uint8) for i in keep])
        assert torch.equal(dec, _cuda(want))
        pos = 0
        for r, i in zip(dres, keep):
            assert (int(r["off"]), int(r["size"])) == (pos, len(files[i])), i
            assert (int(r["chunks_crc"]), int(r["raw_crc"]), int(r["num_chunks"]), int(r["compressed"])) == (
                exp[i]["chunks_crc"], exp[i]["raw_crc"], exp[i]["num_chunks"], 1), i
            pos += len(files[i])


def _group(size_list):
    """A few small files of the size list: five that compress and one (300 bytes) that does not."""
    files, exp = size_list
    idx = [i for i, f in enumerate(files) if len(f) in (300, 600, 1000, 3039, 4095, 5000)]
    return [files[i] for i in idx], [exp[i] for i in idx]


def test_capacity(codec, size_list):
    import torch

    files, exp = _group(size_list)
    buf, offs, lens = fc.pack(files, lead=5)
    d = _cuda(buf)
    need = sum(len(e["stream"]) for e in exp)
    out = torch.zeros(need, dtype=torch.uint8, device="cuda")
    rc, size, _ = codec.compress_files_raw(d, offs, lens, CS, out, out_cap=need - 1)
    assert (rc, size) == (-2, need)
    assert int(out.count_nonzero()) == 0  # nothing written
    rc, size, res_t = codec.compress_files_raw(d, offs, lens, CS, out, out_cap=need)
    assert (rc, size) == (0, need)
    _check(out, codec._results_numpy(res_t), files, exp)
    # the decode side the same way
    keep = [i for i, e in enumerate(exp) if e["compressed"]]
    res = codec._results_numpy(res_t)
    so, ss = [int(res["off"][i]) for i in keep], [int(res["size"][i]) for i in keep]
    total = sum(len(files[i]) for i in keep)
    dout = torch.zeros(total, dtype=torch.uint8, device="cuda")
    rc, size, _, bad = codec.decompress_files_raw(out, so, ss, CS, dout, out_cap=total - 1)
    assert (rc, size) == (-2, total)
    rc, size, _, bad = codec.decompress_files_raw(out, so, ss, CS, dout, out_cap=total)
    assert (rc, size) == (0, total)
    assert dout.cpu().numpy().tobytes() == b"".join(files[i] for i in keep)


def test_rejections(codec, size_list):
    import torch

    files, exp = _group(size_list)
    buf, offs, lens = fc.pack(files, lead=2)
    d = _cuda(buf)
    out = torch.zeros(codec.files_bound(lens, CS), dtype=torch.uint8, device="cuda")
    # compress side: lists that are rejected before any device work
    swapped = offs[:2][::-1] + offs[2:]
    assert codec.compress_files_raw(d, swapped, lens, CS, out)[0] == -1
    overl = [offs[0], offs[0] + lens[0] - 1] + offs[2:]
    assert codec.compress_files_raw(d, overl, lens, CS, out)[0] == -1
    assert codec.compress_files_raw(d, offs, lens, 0, out)[0] == -1
    assert codec.compress_files_raw(d, offs, lens, 1 << 24, out)[0] == -1
    assert codec.compress_files_raw(d, [], [], CS, out)[0] == -1
    # (the 2^31 extent limit is checked on the CPU, tests/cpp/files_plan_check.cpp: no test here
    # passes lengths beyond an allocation)
    rc, size, res_t = codec.compress_files_raw(d, offs, lens, CS, out)
    assert rc == 0
    res = codec._results_numpy(res_t)
    _check(out[:size], res, files, exp)
    stored = [i for i, e in enumerate(exp) if not e["compressed"]]
    good = [i for i, e in enumerate(exp) if e["compressed"]]
    assert len(stored) == 1 and len(good) == 5
    so, ss = [int(x) for x in res["off"]], [int(x) for x in res["size"]]
    dout = torch.zeros(sum(lens) + 64, dtype=torch.uint8, device="cuda")

    def dec(streams, idx, sizes=None):
        sizes = sizes or ss
        rc, size, _, bad = codec.decompress_files_raw(streams, [so[i] for i in idx], [sizes[i] for i in idx], CS, dout)
        return rc, bad

    # a stream that is not smaller than its file: the reference's end-of-entry check rejects it
    rc, bad = dec(out, good[:2] + stored + good[2:])
    assert (rc, bad) == (-1, 2)
    # a stream shortened by one byte
    k = 3
    short = list(ss)
    short[good[k]] -= 1
    assert dec(out, good, short) == (-1, k)
    # a header's encoded_size field zeroed, in a copy
    bad_hdr = out.clone()
    p = so[good[1]] + 3 + 260
    bad_hdr[p:p + 4] = 0
    assert dec(bad_hdr, good) == (-1, 1)
    # two bad files: the lower index is reported
    short[good[4]] -= 1
    assert dec(bad_hdr, good, short) == (-1, 1)
    assert dec(out, good, short) == (-1, k)
    # an empty stream
    empty = list(ss)
    empty[good[0]] = 0
    assert dec(out, good, empty) == (-1, 0)
    # the same call without the bad files succeeds
    rc, size, dres_t, bad = codec.decompress_files_raw(out, [so[i] for i in good], [ss[i] for i in good], CS, dout)
    assert (rc, bad) == (0, 0xFFFFFFFF)
    assert dout[:size].cpu().numpy().tobytes() == b"".join(files[i] for i in good)
    with pytest.raises(ValueError) as ei:
        codec.decompress_files(out, so, ss, CS)
    assert ei.value.bad_file == stored[0]


def test_agrees_with_single_file_call(codec, size_list):
    files, _ = size_list
    pick = [i for i, f in enumerate(files) if len(f) in (1, 300, 4097, 262145, 524295)]
    assert len(pick) == 5
    sub = [files[i] for i in pick]
    buf, offs, lens = fc.pack(sub, lead=7)
    d = _cuda(buf)
    out, res = codec.compress_files(d, offs, lens, CS)
    out_h = out.cpu().numpy()
    for r, o, n in zip(res, offs, lens):
        s1, crc1, comp1 = codec.compress_chunks(d[o:o + n], CS)
        assert out_h[int(r["off"]):int(r["off"] + r["size"])].tobytes() == s1.cpu().numpy().tobytes(), n
        assert (int(r["chunks_crc"]), int(r["compressed"])) == (crc1, int(comp1)), n


def test_explicit_stream(codec, size_list):
    """Both calls on a caller-supplied stream, inputs produced on that stream."""
    import torch

    files, exp = _group(size_list)
    buf, offs, lens = fc.pack(files, align=16)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = _cuda(buf)
        out, res = codec.compress_files(d, offs, lens, CS, stream=s)
        keep = [i for i, e in enumerate(exp) if e["compressed"]]
        dec, dres = codec.decompress_files(out, [int(res["off"][i]) for i in keep], [int(res["size"][i]) for i in keep], CS, stream=s)
        dec_h = dec.cpu().numpy().tobytes()
    s.synchronize()
    _check(out, res, files, exp)
    assert dec_h == b"".join(files[i] for i in keep)
    assert [int(x) for x in dres["chunks_crc"]] == [exp[i]["chunks_crc"] for i in keep]
    assert [int(x) for x in dres["raw_crc"]] == [exp[i]["raw_crc"] for i in keep]


def test_default_stream_complete_on_return(bra, codec, small_block):
    """Without a stream the call runs on the context's stream and is complete when it returns: the
    results are read with .cpu() on torch's default stream straight after it, with no synchronise,
    right behind a long call of another geometry."""
    import torch

    files, exp = small_block
    buf, offs, lens = fc.pack(files, lead=1)
    d = _cuda(buf)
    busy = torch.from_numpy(bra.synth_fill(0, 8 << 20, 1 << 18)).cuda()
    out = torch.empty(codec.files_bound(lens, 4096), dtype=torch.uint8, device="cuda")
    for _ in range(3):
        res_t = torch.zeros(len(files) * 32, dtype=torch.uint8, device="cuda")
        out.zero_()
        codec.encode(busy, 1 << 18)
        rc, size, res_t = codec.compress_files_raw(d, offs, lens, 4096, out, results=res_t)
        res = res_t.cpu().numpy().view(np.dtype(bra.FILE_RESULT_FIELDS))
        assert rc == 0
        _check(out[:size], res, files, exp)
