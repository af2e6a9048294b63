"""Wide first BWT split, sparse-prefix form: micro-benchmark driver (measurement only).

    [KIND=0|2] [NB=256] [WL0W_SO=path] python scripts/micro/wl0w.py [tile ...]      tiles: 8192 16384 32768

Builds libwl0w.so from wl0w.hip if needed.  Feeds NB synthetic blocks of 1 MiB, packed on the host
the way k_pack packs them, through the prefix-map, histogram and scatter kernels; the offsets come
from a host-side (torch) scan of the histogram rows.  One JSON line per tile size: ms per launch of
each kernel (HIP events) and whether the scatter wrote every slot exactly once, in prefix order,
with the payloads, digit bytes and job words the level machinery expects (two blocks checked
element by element on the CPU)."""
import ctypes
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
bra = importlib.import_module("br-archive_amd")
import wide_l0  # noqa: E402

so = os.environ.get("WL0W_SO", os.path.join(HERE, "libwl0w.so"))
if not os.path.exists(so):
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "wl0w.hip")])
lib = ctypes.CDLL(so)


class WArgs(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("inp", "packed", "inv", "bm", "rkw", "nbins", "rows", "goff", "opay", "odig", "p32")] + \
               [(k, ctypes.c_uint32) for k in ("n", "b", "pstride", "nblocks", "bs", "ntot")]


lib.wl0w_launch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(WArgs), ctypes.c_void_p]
lib.wl0w_scatter_lds.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_uint]
lib.wl0w_scatter_lds.restype = ctypes.c_uint

n, nb = 1 << 20, int(os.environ.get("NB", "256"))
kind = int(os.environ.get("KIND", bra.SYNTH_TEXT))
JOB_WG, EXT_BITS, FLAG = 1024, 384, 1 << 31
h = bra.synth_fill(kind, n * nb, n).reshape(nb, n)

# pack every block: alphabet ranks, b bits per character MSB first, the first EXT_BITS bits again
bits_of = [wide_l0.pack_bits(h[k])[1] for k in range(nb)]
b = bits_of[0]
assert all(x == b for x in bits_of), "blocks with different bits per character"
pstride = (n * b // 8 + 96 + 15) // 16 * 16
packed = np.zeros((nb, pstride), np.uint8)
inv = np.zeros((nb, 256), np.uint8)
for k in range(nb):
    codes, _ = wide_l0.pack_bits(h[k])
    vals = np.unique(h[k])
    inv[k, :vals.size] = vals
    bits = ((codes[:, None] >> np.arange(b - 1, -1, -1)) & 1).astype(np.uint8).ravel()
    packed[k, :(n * b + EXT_BITS) // 8] = np.packbits(np.concatenate([bits, bits[:EXT_BITS]]))

dev = "cuda"
d_in, d_pk, d_inv = torch.from_numpy(h).to(dev), torch.from_numpy(packed).to(dev), torch.from_numpy(inv).to(dev)
d_bm = torch.zeros(nb, 2048, dtype=torch.int32, device=dev)
d_rkw = torch.zeros(nb, 2048, dtype=torch.int16, device=dev)
d_nbins = torch.zeros(nb + 1, dtype=torch.int32, device=dev)
opay = torch.empty(n * nb, dtype=torch.int64, device=dev)
odig = torch.empty(n * nb, dtype=torch.uint8, device=dev)
p32 = torch.empty(n * nb, dtype=torch.int32, device=dev)
stream = torch.cuda.current_stream().cuda_stream
a = WArgs(inp=d_in.data_ptr(), packed=d_pk.data_ptr(), inv=d_inv.data_ptr(), bm=d_bm.data_ptr(), rkw=d_rkw.data_ptr(), nbins=d_nbins.data_ptr(),
          rows=0, goff=0, opay=opay.data_ptr(), odig=odig.data_ptr(), p32=p32.data_ptr(), n=n, b=b, pstride=pstride, nblocks=nb, bs=4, ntot=n * nb)


def launch(which, tile):
    rc = lib.wl0w_launch(which, tile, ctypes.byref(a), stream)
    assert rc == 0, (which, tile, rc)


def timed(which, tile, reps=10):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(3):
        launch(which, tile)
    ev[0].record()
    for _ in range(reps):
        launch(which, tile)
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def key_bytes(k, idx):
    """key bytes 0..7 of rotations idx of block k as uint64 (CPU)."""
    P = packed[k].astype(np.uint64)
    bit = idx.astype(np.int64) * b
    off, sh = bit >> 3, (bit & 7).astype(np.uint64)
    hi = np.zeros(idx.size, np.uint64)
    for j in range(8):
        hi = (hi << np.uint64(8)) | P[off + j]
    return (hi << sh) | (P[off + 8] >> (np.uint64(8) - sh))


def check_block(k, idx, flag, pay, dig, w32):
    """slot order, payloads, digit bytes and job words of block k against the CPU."""
    kk = key_bytes(k, idx)
    pfx = (kk >> np.uint64(48)).astype(np.int64)
    lb = h[k][(idx - 1) % n].astype(np.uint64)
    want = ((kk << np.uint64(16)) & np.uint64(0xFFFFFFFF00000000)) | (lb << np.uint64(24)) | idx.astype(np.uint64)
    return bool(np.all(np.diff(pfx) >= 0)
                and np.array_equal(pay.view(np.uint64)[flag], want[flag])
                and np.array_equal(dig[flag], ((kk >> np.uint64(40)) & np.uint64(0xFF)).astype(np.uint8)[flag])
                and np.array_equal(w32.view(np.uint32)[~flag], (want & np.uint64(0xFFFFFFFF)).astype(np.uint32)[~flag]))


for tile in [int(x) for x in sys.argv[1:]] or [8192, 16384, 32768]:
    tpb = n // tile
    d_bm.zero_()
    d_nbins.zero_()
    launch(0, tile)
    torch.cuda.synchronize()
    nbins = d_nbins.cpu().numpy()
    B0 = wide_l0.prefix_count(h[0])
    bs = (int(nbins[nb]) + 3) // 4 * 4
    res = {"tile": tile, "kind": kind, "blocks": nb, "bits": b, "B_max": int(nbins[nb]), "B_min": int(nbins[:nb].min()), "B_block0_ok": bool(nbins[0] == B0),
           "scatter_lds": int(lib.wl0w_scatter_lds(tile, b, bs))}
    a.bs = bs
    rows = torch.zeros(nb * tpb, bs, dtype=torch.int16, device=dev)
    a.rows = rows.data_ptr()
    launch(1, tile)
    torch.cuda.synchronize()
    cnt = rows.view(nb, tpb, bs).to(torch.int32)  # counts <= 32768 would wrap int16 only at exactly 32768: masked below
    cnt = cnt & 0xFFFF
    tot = cnt.sum(1)
    pf0 = wide_l0.prefix16(h[0]).astype(np.int64)
    res["hist_ok"] = bool((tot.sum(1) == n).all()) and bool(np.array_equal(tot[0, :B0].cpu().numpy(), np.bincount(pf0, minlength=65536)[np.unique(pf0)]))
    sub = torch.cumsum(tot, 1) - tot + (torch.arange(nb, device=dev) * n).view(nb, 1)
    goff = (sub.view(nb, 1, bs) + torch.cumsum(cnt, 1) - cnt).to(torch.int64)
    flag = tot > JOB_WG
    goff = torch.where(flag.view(nb, 1, bs), goff - FLAG, goff).to(torch.int32).contiguous()  # bit 31 set, as a signed word
    a.goff = goff.data_ptr()
    del cnt, sub
    if res["hist_ok"]:
        opay.fill_(-1)
        p32.fill_(-1)
        launch(2, tile)
        torch.cuda.synchronize()
        sflag = torch.repeat_interleave(flag.view(-1), tot.view(-1).long())
        idx = torch.where(sflag, opay & 0xFFFFFF, p32.long() & 0xFFFFFF).view(nb, n)
        written = bool(torch.where(sflag, opay != -1, p32 != -1).all())
        perm = bool((torch.sort(idx, dim=1).values == torch.arange(n, device=dev)).all())
        cpu_ok = all(check_block(k, idx[k].cpu().numpy(), sflag.view(nb, n)[k].cpu().numpy(), opay.view(nb, n)[k].cpu().numpy(),
                                 odig.view(nb, n)[k].cpu().numpy(), p32.view(nb, n)[k].cpu().numpy()) for k in sorted({0, nb - 1}))
        res.update(exact_once=written and perm, cpu_check=cpu_ok, continue_elems=int(tot[flag].sum()))
        del sflag, idx
        res["ms_bins"] = timed(0, tile)
        res["ms_hist"] = timed(1, tile)
        res["ms_scatter"] = timed(2, tile)
        res["ms_sum"] = res["ms_bins"] + res["ms_hist"] + res["ms_scatter"]
    print(json.dumps(res), flush=True)
    del rows, goff
