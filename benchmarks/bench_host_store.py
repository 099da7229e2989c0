"""The slot-table host copies (copy_blocks_{to,from}_host_slots, what HostBlockStore runs on) next to the dense entries
(copy_blocks_to_host / _from_host and the MXFP8 pair), alternating run by run in one process.

Llama-3-8B per layer (32 layers, K/V: 64 regions, 32 KiB blocks of bf16, a 2 MiB row per block); n = 8, 64, 512 blocks. The
dense image is n rows; the arena has 4n rows and the n slots are scattered over it (a random subset in random order, slot 0
and the last slot among them). The row of a block is contiguous on both paths, so only the order of the rows differs: the
expectation is that the slot path's median is no lower than the dense path's slowest run. One JSON line per size, codec
("raw", "mxfp8") and direction ("offload": device -> host, "restore": host -> device):
  image_bytes          what crosses the link (n * 64 records)
  dense_GBps/slot_GBps image_bytes over the device time of each run (events around the launches alone), --runs of each, the
                       two paths taking turns run by run after --warmup unrecorded turns
  *_median_GBps, dense_min_GBps, slot_median_ge_dense_min   the expectation above
  ok                   the slot rows equal the dense rows byte for byte, and what a restore from the slots leaves on the
                       device equals what the dense restore leaves

Usage: python benchmarks/bench_host_store.py [--runs 5] [--warmup 2] [--sizes 8,64,512] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("KVCACHED_PAGE_PREALLOC_ENABLED", "false")
os.environ.setdefault("KVCACHED_IPC_NAME", f"kvc_bench_host_store_{os.getpid()}")
os.environ.setdefault("KVCACHED_LOG_LEVEL", "ERROR")

import numpy as np  # noqa: E402
import torch  # noqa: E402

PAGE = 2 << 20
DEV = "cuda:0"
LAYERS, BLOCK_TOKENS, CELL = 32, 16, 2048
DTYPE = torch.bfloat16


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _alternating_ms(fns, runs, warmup):
    """Device time of every run of each fn, the fns taking turns run by run."""
    out = [[] for _ in fns]
    for i in range(warmup + runs):
        for k, fn in enumerate(fns):
            ms = _timed(fn)
            if i >= warmup:
                out[k].append(ms)
    return out


def run(sizes, runs: int, warmup: int):
    import kvcached_amd.kv_cache_manager as kcm
    from kvcached_amd import capi, vmm_ops
    kcm.CONTIGUOUS_LAYOUT = False
    vmm_ops.init_kvcached(DEV, PAGE, False)
    bmem = BLOCK_TOKENS * CELL
    n_pages = 2 * max(sizes) * bmem // PAGE + 2
    nb = n_pages * (PAGE // bmem)
    raw = vmm_ops.create_kv_tensors(n_pages * PAGE * 2, 1, DEV, LAYERS, 2, 0, False)
    m = kcm.KVCacheManager(num_blocks=nb, block_size=BLOCK_TOKENS, cell_size=CELL, num_layers=LAYERS)
    assert m._post_init_done.wait(10)
    bases, bb = m._block_geometry()
    R = len(bases)
    views = []
    for t in raw:
        u = t.view(torch.uint8)
        views += [u[:nb * bb].view(nb, bb), u[u.numel() // 2:u.numel() // 2 + nb * bb].view(nb, bb)]
    assert len(views) == R
    codecs = {"raw": 0, "mxfp8": capi.KVC_CODEC_MXFP8_BF16}
    st = torch.cuda.Stream()   # (in the C ABI, NULL names the library's own stream)
    stream = st.cuda_stream
    lines = []
    try:
        for n in sizes:
            with torch.cuda.stream(st):
                ids, other = m.alloc(n), m.alloc(n)                    # `other`: where the restores go
                g = torch.Generator(device=DEV).manual_seed(n)
                ids_t, other_t = torch.tensor(ids, device=DEV), torch.tensor(other, device=DEV)
                for v in views:
                    v[ids_t] = torch.randn(n, bb // 2, device=DEV, generator=g).to(DTYPE).view(torch.uint8)
                torch.cuda.synchronize()
                n_slots = 4 * n
                rng = np.random.default_rng(n)
                slots = np.concatenate([rng.choice(np.arange(1, n_slots - 1), size=n - 2, replace=False), [0, n_slots - 1]])
                rng.shuffle(slots)
                slots = [int(s) for s in slots]
                for name, codec in codecs.items():
                    rec = capi.codec_record_bytes(codec, bb) if codec else bb
                    row, image = R * rec, n * R * rec
                    dense = torch.empty(image, dtype=torch.uint8, pin_memory=True)
                    arena = torch.empty(n_slots * row, dtype=torch.uint8, pin_memory=True)
                    arena.fill_(0)                                     # every page of it touched before the clock runs
                    dense.fill_(0)
                    if codec:
                        dense_to = lambda: capi.encode_blocks_to_host(0, ids, bb, codec, dense.data_ptr(), stream, sync=False)  # noqa: E731
                        dense_from = lambda: capi.decode_blocks_from_host(0, other, bb, codec, dense.data_ptr(), stream, sync=False)  # noqa: E731
                    else:
                        dense_to = lambda: capi.copy_blocks_to_host(0, ids, bb, dense.data_ptr(), stream, sync=False)  # noqa: E731
                        dense_from = lambda: capi.copy_blocks_from_host(0, other, bb, dense.data_ptr(), stream, sync=False)  # noqa: E731
                    slot_to = lambda: capi.copy_blocks_to_host_slots(0, ids, slots, bb, codec, arena.data_ptr(), n_slots,  # noqa: E731
                                                                     stream, sync=False)
                    slot_from = lambda: capi.copy_blocks_from_host_slots(0, other, slots, bb, codec, arena.data_ptr(),  # noqa: E731
                                                                         n_slots, stream, sync=False)
                    times = {"offload": _alternating_ms([dense_to, slot_to], runs, warmup),
                             "restore": _alternating_ms([dense_from, slot_from], runs, warmup)}
                    torch.cuda.synchronize()
                    ok = torch.equal(arena.view(n_slots, row)[torch.tensor(slots)], dense.view(n, row))
                    dense_from()
                    torch.cuda.synchronize()
                    left = [v[other_t].clone() for v in views]
                    for v in views:
                        v[other_t] = 0
                    slot_from()
                    torch.cuda.synchronize()
                    ok = ok and all(torch.equal(v[other_t], w) for v, w in zip(views, left))
                    for direction, (d_ms, s_ms) in times.items():
                        d = [round(image / ms / 1e6, 2) for ms in d_ms]
                        s = [round(image / ms / 1e6, 2) for ms in s_ms]
                        line = {"bench": "host_store", "codec": name, "direction": direction, "regions": R, "block_bytes": bb,
                                "n_blocks": n, "n_slots": n_slots, "image_bytes": image, "dense_GBps": d, "slot_GBps": s,
                                "dense_median_GBps": statistics.median(d), "slot_median_GBps": statistics.median(s),
                                "dense_min_GBps": min(d), "slot_median_ge_dense_min": statistics.median(s) >= min(d),
                                "ok": bool(ok), "runs": runs, "warmup": warmup}
                        print(json.dumps(line), flush=True)
                        lines.append(line)
                    del dense, arena
                m.free(ids + other)
    finally:
        del m
        vmm_ops.shutdown_kvcached()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="8,64,512")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_host_store needs the MI355X"
    lines = run([int(s) for s in a.sizes.split(",")], a.runs, a.warmup)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    if not all(line["ok"] for line in lines):
        sys.exit(1)


if __name__ == "__main__":
    main()
