"""`bench.py --dump-outputs DIR`: the arrays written after the timed steps.

CPU: dump_outputs on host tensors, the whole payload and the seeded sample of a larger one, the
per-block sums against numpy.  GPU: one plain bench run on a small ragged input; its line carries
the headline fields only and its dump equals a direct encode of the same synthetic input."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAMES = ("crc32c", "headers", "offsets", "payload", "payload_block_sums")


def _load(d):
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in NAMES)
    z = {n: np.load(os.path.join(d, n + ".npy"), allow_pickle=False) for n in NAMES}
    assert all(a.dtype in (np.float32, np.float64) for a in z.values())
    return z


def _block_sums(pay, off):
    p = pay.astype(np.int64)
    w = np.arange(p.size, dtype=np.int64) % 65521 + 1
    return np.array([[p[a:b].sum(), (p * w)[a:b].sum()] for a, b in zip(off[:-1], off[1:])], dtype=np.float64)


@pytest.mark.parametrize("cap", [None, 1000])
def test_dump_outputs_arrays(tmp_path, monkeypatch, cap):
    import torch

    import bench

    rng = np.random.default_rng(1)
    nbg = 5
    off = np.concatenate([[0], np.cumsum(rng.integers(1, 70000, nbg))]).astype(np.int64)
    pay = rng.integers(0, 256, int(off[-1]) + 777, dtype=np.uint8)  # capacity past the last offset
    hdr = rng.integers(0, 256, (nbg, 268), dtype=np.uint8)
    if cap is not None:
        monkeypatch.setattr(bench, "DUMP_PAYLOAD_MAX", cap)
    d = str(tmp_path / "out")
    bench.dump_outputs(d, torch.from_numpy(hdr), torch.from_numpy(off), torch.from_numpy(pay), torch.tensor([-5], dtype=torch.int32), nbg)
    z = _load(d)
    n = int(off[-1])
    assert z["crc32c"].tolist() == [2.0 ** 32 - 5]
    assert np.array_equal(z["headers"], hdr) and np.array_equal(z["offsets"], off)
    assert np.array_equal(z["payload_block_sums"], _block_sums(pay[:n], off))
    if cap is None:
        assert np.array_equal(z["payload"], pay[:n])
    else:
        idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, n, size=cap, dtype=np.int64))
        assert np.array_equal(z["payload"], pay[:n][idx])


@pytest.mark.gpu
def test_plain_bench_line_and_dump(tmp_path):
    import torch

    bra = importlib.import_module("br-archive_amd")
    bs, total = 1 << 20, (2 << 20) + 12345  # three blocks, the last one short
    d = str(tmp_path / "out")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--bytes-per-gpu", str(total),
           "--dump-outputs", d]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert (line["steps"], line["warmup"], line["unit"], line["dtype"], line["higher_is_better"]) == (2, 1, "GB/s", "u8", True)
    assert line["ms_per_step"] > 0 and abs(line["value"] - total / line["ms_per_step"] / 1e6) <= 0.02 * line["value"]
    assert line["roofline"] is None and line["cpu_baseline"] is None and "reference_check" not in line
    z = _load(d)
    codec = bra.BlockCodec(0)
    data = torch.from_numpy(bra.synth_fill(bra.SYNTH_TEXT, total, bs)).to("cuda:0")
    hdr, off, pay = codec.encode(data, bs)
    crc = codec.chunks_crc32c(data, hdr, bs)
    torch.cuda.synchronize()
    hdr, off, pay = hdr.cpu().numpy(), off.cpu().numpy(), pay.cpu().numpy()
    codec.close()
    n = int(off[-1])
    assert n == line["pipeline"]["payload_bytes"]
    assert z["crc32c"].tolist() == [float(crc)]
    assert np.array_equal(z["headers"], hdr) and np.array_equal(z["offsets"], off)
    assert np.array_equal(z["payload"], pay[:n])
    assert np.array_equal(z["payload_block_sums"], _block_sums(pay[:n], off))
