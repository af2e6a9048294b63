#!/usr/bin/env python3
"""Many small files: one bra_gpu_compress_files / bra_gpu_decompress_files call against a loop of
bra_gpu_compress_chunks / bra_gpu_decompress_chunks per file (the only way before the files calls).

Input: synthetic text files with seeded log-uniform sizes between 1 KiB and 64 KiB, resident in
HBM.  Both forms run in this one process, warm, on the NULL stream (complete on return) inside a
host clock; the figure of each is the median of the runs.  The single call is timed twice: on the
same list every run (the context's per-geometry caches hit) and on a list that differs from the
previous call's (they miss, as for an archiver).  One JSON document goes to --out and its summary
line to stdout (files/s: loop, one call, one call on a new list); the exit status is 1 when the
single call is not faster than the loop.

    python scripts/files_bench.py [--files 4096] [--runs 5] [--out profiles/files_bench.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "files_bench.json"))
    a = ap.parse_args()
    import torch

    bra = importlib.import_module("br-archive_amd")
    lib, cs = bra.lib, bra.MAX_CHUNK_SIZE
    rng = np.random.default_rng(a.seed)
    lens = [int(x) for x in np.exp(rng.uniform(np.log(1024), np.log(65536), a.files))]
    offs = [int(x) for x in np.concatenate([[0], np.cumsum(lens)[:-1]])]
    total = sum(lens)
    d = torch.from_numpy(bra.synth_fill(bra.SYNTH_TEXT, total, 1 << 16)).cuda()
    codec = bra.BlockCodec(0)
    cap = codec.files_bound(lens, cs)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    out1 = torch.empty(cap, dtype=torch.uint8, device="cuda")
    res_t = torch.empty(a.files * 32, dtype=torch.uint8, device="cuda")
    size, crc = C.c_uint64(), C.c_uint32()

    def loop_compress():
        pos = 0
        for o, n in zip(offs, lens):
            rc = lib.bra_gpu_compress_chunks(codec.ctx, d.data_ptr() + o, n, cs, out1.data_ptr() + pos, cap - pos, C.byref(size), C.byref(crc), None)
            assert rc >= 0, rc
            pos += size.value
        return pos

    def one_compress(skip=0):
        rc, sz, _ = codec.compress_files_raw(d, offs[skip:], lens[skip:], cs, out, results=res_t)
        assert rc == 0, rc
        return sz

    def timed_new_list(fn):
        """As timed(), but every call gets a list that differs from the previous call's (with or
        without the first file), so the per-geometry caches of the context miss as they do for an
        archiver, whose every call has a new list."""
        fn(1)
        fn(0)
        ts = []
        for k in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(1 - k % 2)
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), ts

    def timed(fn):
        fn()  # warm: allocations, geometry caches
        ts = []
        for _ in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), ts

    csize = one_compress()
    assert loop_compress() == csize and torch.equal(out[:csize], out1[:csize]), "the two forms disagree"
    res = codec._results_numpy(res_t)
    sel = np.flatnonzero(res["compressed"] == 1)
    so, ss = [int(x) for x in res["off"][sel]], [int(x) for x in res["size"][sel]]
    dlen = [lens[i] for i in sel]
    dtotal = sum(dlen)
    dec = torch.empty(dtotal + 16, dtype=torch.uint8, device="cuda")
    dec1 = torch.empty(dtotal + 16, dtype=torch.uint8, device="cuda")
    dres_t = torch.empty(max(len(sel), 1) * 32, dtype=torch.uint8, device="cuda")

    def loop_decompress():
        pos = 0
        for o, n in zip(so, ss):
            rc = lib.bra_gpu_decompress_chunks(codec.ctx, out.data_ptr() + o, n, cs, dec1.data_ptr() + pos, dtotal - pos, C.byref(size), 0, C.byref(crc),
                                               None)
            assert rc == 0, rc
            pos += size.value
        return pos

    def one_decompress(skip=0):
        rc, sz, _, bad = codec.decompress_files_raw(out, so[skip:], ss[skip:], cs, dec, results=dres_t, out_cap=dtotal)
        assert rc == 0, (rc, bad)
        return sz

    assert one_decompress() == dtotal and loop_decompress() == dtotal and torch.equal(dec[:dtotal], dec1[:dtotal]), "the two decodes disagree"
    t_cl, r_cl = timed(loop_compress)
    t_c1, r_c1 = timed(one_compress)
    t_cn, r_cn = timed_new_list(one_compress)
    csize = one_compress()  # `out` holds the whole list's streams again
    t_dl, r_dl = timed(loop_decompress)
    t_d1, r_d1 = timed(one_decompress)
    t_dn, r_dn = timed_new_list(one_decompress)

    def rate(t, files, nbytes):
        return {"seconds": t, "files_per_s": files / t, "GB_per_s": nbytes / t / 1e9}

    doc = {
        "files": a.files, "input_bytes": total, "stream_bytes": int(csize), "compressed_files": int(len(sel)), "runs": a.runs, "seed": a.seed,
        "device": torch.cuda.get_device_name(0), "library": bra.version(),
        "compress": {"per_file_loop": rate(t_cl, a.files, total), "one_call": rate(t_c1, a.files, total),
                     "one_call_new_list": rate(t_cn, a.files, total), "speedup": t_cl / t_c1, "speedup_new_list": t_cl / t_cn,
                     "runs_s": {"per_file_loop": r_cl, "one_call": r_c1, "one_call_new_list": r_cn}},
        "decompress": {"per_file_loop": rate(t_dl, len(sel), dtotal), "one_call": rate(t_d1, len(sel), dtotal),
                       "one_call_new_list": rate(t_dn, len(sel), dtotal), "speedup": t_dl / t_d1, "speedup_new_list": t_dl / t_dn,
                       "runs_s": {"per_file_loop": r_dl, "one_call": r_d1, "one_call_new_list": r_dn}},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"files": a.files, "compress_speedup": round(t_cl / t_c1, 2), "decompress_speedup": round(t_dl / t_d1, 2),
                      "compress_files_per_s": [round(a.files / t_cl), round(a.files / t_c1), round(a.files / t_cn)],
                      "decompress_files_per_s": [round(len(sel) / t_dl), round(len(sel) / t_d1), round(len(sel) / t_dn)]}))
    codec.close()
    return 0 if max(t_c1, t_cn) < t_cl and max(t_d1, t_dn) < t_dl else 1


if __name__ == "__main__":
    sys.exit(main())
