"""Offload / restore of live KV blocks through the MXFP8 codec (encode_blocks_to_host / decode_blocks_from_host) next to
the raw copies (copy_blocks_to_host / copy_blocks_from_host), alternating in one process, against the host link itself.

The link is the limit of both paths; the codec puts 33/64 of the bytes on it. One JSON line per geometry, size and path
("raw", "mxfp8"). Geometries and sizes as benchmarks/bench_offload.py: Llama-3-8B (32 layers, K/V, 32 KiB blocks of
bf16) per layer (64 regions) and contiguous (1 region, 2 MiB per block); n = 8, 64, 512 blocks (512 blocks = 1 GiB).
Per line:
  logical_bytes / image_bytes        the 16-bit bytes of the blocks / the bytes of the host image (what crosses the link)
  offload_copy_ms / restore_copy_ms  device events around the kernel launches alone (median of --steps; the two paths
                                     take turns step by step, so drift of the machine hits both alike)
  *_logical_GBps                     logical_bytes over that time
  *_link_GBps                        image_bytes over that time
  link_d2h_GBps / link_h2d_GBps      the link ceiling in the same process: one contiguous device tensor of image_bytes
                                     copied to / from a pinned tensor with copy_(non_blocking=True)
  offload_vs_link / restore_vs_link  *_link_GBps over that ceiling
  ok                                 raw: the restored bytes are the offloaded ones; mxfp8: every restored element is within
                                     max(|x| * 2^-4, 2^(se - 10)) of x, se the group's shared exponent (the bits themselves
                                     are pinned by tests/test_gpu_kv_codec.py)

Usage: python benchmarks/bench_offload_mxfp8.py [--steps 10] [--warmup 3] [--sizes 8,64,512] [--out FILE]
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
os.environ.setdefault("KVCACHED_IPC_NAME", f"kvc_bench_offload_mxfp8_{os.getpid()}")
os.environ.setdefault("KVCACHED_LOG_LEVEL", "ERROR")

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


def _alternating_ms(fns, steps, warmup):
    """Median device time of each fn, the fns taking turns step by step."""
    out = [[] for _ in fns]
    for i in range(warmup + steps):
        for k, fn in enumerate(fns):
            ms = _timed(fn)
            if i >= warmup:
                out[k].append(ms)
    return [statistics.median(o) for o in out]


def _within_bound(x, y):
    """Every y within max(|x| * 2^-4, 2^(se - 10)) of x; se: the smallest integer with amax * 2^-se <= 448, per 32 elements."""
    xd, yd = x.reshape(-1, 32).double(), y.reshape(-1, 32).double()
    amax = xd.abs().amax(1, keepdim=True)
    se = torch.ceil(torch.log2(amax.clamp_min(2.0 ** -300) / 448.0)).clamp(-127, 127)
    bound = torch.maximum(xd.abs() * 2.0 ** -4, torch.exp2(se - 10).expand_as(xd))
    return bool(((xd - yd).abs() <= bound).all())


def run_geometry(contiguous: bool, sizes, steps: int, warmup: int):
    import kvcached_amd.kv_cache_manager as kcm
    from kvcached_amd import capi, vmm_ops
    kcm.CONTIGUOUS_LAYOUT = contiguous
    vmm_ops.init_kvcached(DEV, PAGE, contiguous)
    bmem = BLOCK_TOKENS * CELL
    n_pages = 2 * max(sizes) * bmem // PAGE + 2
    nb = n_pages * (PAGE // bmem)
    raw = vmm_ops.create_kv_tensors(n_pages * PAGE * 2, 1, DEV, LAYERS, 2, 0, False)
    m = kcm.KVCacheManager(num_blocks=nb, block_size=BLOCK_TOKENS, cell_size=CELL, num_layers=LAYERS)
    assert m._post_init_done.wait(10)
    bases, bb = m._block_geometry()
    R = len(bases)
    if contiguous:
        views = [raw[0].view(torch.uint8)[:nb * bb].view(nb, bb)]
    else:
        views = []
        for t in raw:
            u = t.view(torch.uint8)
            views += [u[:nb * bb].view(nb, bb), u[u.numel() // 2:u.numel() // 2 + nb * bb].view(nb, bb)]
    assert len(views) == R
    codec = capi.KVC_CODEC_MXFP8_BF16
    rec = capi.codec_record_bytes(codec, bb)
    st = torch.cuda.Stream()   # (in the C ABI, NULL names the library's own stream)
    stream = st.cuda_stream
    lines = []
    try:
        for n in sizes:
            with torch.cuda.stream(st):
                ids = m.alloc(n)
                other = m.alloc(n)                                 # where the restores go
                g = torch.Generator(device=DEV).manual_seed(n)
                ids_t, other_t = torch.tensor(ids, device=DEV), torch.tensor(other, device=DEV)
                for v in views:
                    v[ids_t] = torch.randn(n, bb // 2, device=DEV, generator=g).to(DTYPE).view(torch.uint8)
                torch.cuda.synchronize()
                logical = n * R * bb
                image = {"raw": logical, "mxfp8": n * R * rec}
                host = {k: torch.empty(b, dtype=torch.uint8, pin_memory=True) for k, b in image.items()}
                to_host = {"raw": lambda: capi.copy_blocks_to_host(0, ids, bb, host["raw"].data_ptr(), stream, sync=False),
                           "mxfp8": lambda: capi.encode_blocks_to_host(0, ids, bb, codec, host["mxfp8"].data_ptr(), stream,
                                                                        sync=False)}
                from_host = {"raw": lambda: capi.copy_blocks_from_host(0, other, bb, host["raw"].data_ptr(), stream, sync=False),
                             "mxfp8": lambda: capi.decode_blocks_from_host(0, other, bb, codec, host["mxfp8"].data_ptr(),
                                                                           stream, sync=False)}
                paths = ["raw", "mxfp8"]
                d2h = dict(zip(paths, _alternating_ms([to_host[p] for p in paths], steps, warmup)))
                h2d = dict(zip(paths, _alternating_ms([from_host[p] for p in paths], steps, warmup)))
                ok = {}
                for p in paths:                                    # what the last restore of each path left behind
                    from_host[p]()
                    torch.cuda.synchronize()
                    if p == "raw":
                        ok[p] = all(torch.equal(v[other_t], v[ids_t]) for v in views)
                    else:
                        ok[p] = all(_within_bound(v[ids_t].view(DTYPE), v[other_t].view(DTYPE)) for v in views)
                # the link ceiling at each image's size, the two sizes taking turns like the paths
                dev = {p: torch.empty(image[p], dtype=torch.uint8, device=DEV) for p in paths}
                pin = {p: torch.empty(image[p], dtype=torch.uint8, pin_memory=True) for p in paths}
                link_d2h = dict(zip(paths, _alternating_ms([(lambda p=p: pin[p].copy_(dev[p], non_blocking=True))
                                                            for p in paths], steps, warmup)))
                link_h2d = dict(zip(paths, _alternating_ms([(lambda p=p: dev[p].copy_(pin[p], non_blocking=True))
                                                            for p in paths], steps, warmup)))
                del dev, pin
                gbps = lambda nbytes, ms: round(nbytes / ms / 1e6, 2)   # noqa: E731
                for p in paths:
                    line = {
                        "bench": "offload_mxfp8", "path": p, "layout": "contiguous" if contiguous else "per_layer",
                        "regions": R, "block_bytes": bb, "n_blocks": n, "logical_bytes": logical, "image_bytes": image[p],
                        "offload_copy_ms": round(d2h[p], 4), "restore_copy_ms": round(h2d[p], 4),
                        "offload_logical_GBps": gbps(logical, d2h[p]), "restore_logical_GBps": gbps(logical, h2d[p]),
                        "offload_link_GBps": gbps(image[p], d2h[p]), "restore_link_GBps": gbps(image[p], h2d[p]),
                        "link_d2h_GBps": gbps(image[p], link_d2h[p]), "link_h2d_GBps": gbps(image[p], link_h2d[p]),
                        "offload_vs_link": round(link_d2h[p] / d2h[p], 3), "restore_vs_link": round(link_h2d[p] / h2d[p], 3),
                        "ok": bool(ok[p]), "steps": steps, "warmup": warmup,
                    }
                    if p == "mxfp8":
                        line["offload_logical_vs_raw"] = round(d2h["raw"] / d2h[p], 3)
                        line["restore_logical_vs_raw"] = round(h2d["raw"] / h2d[p], 3)
                    print(json.dumps(line), flush=True)
                    lines.append(line)
                m.free(ids + other)
                del host
    finally:
        del m
        vmm_ops.shutdown_kvcached()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="8,64,512")
    ap.add_argument("--layouts", default="per_layer,contiguous")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_offload_mxfp8 needs the MI355X"
    sizes = [int(s) for s in a.sizes.split(",")]
    lines = []
    for layout in a.layouts.split(","):
        lines += run_geometry(layout == "contiguous", sizes, a.steps, a.warmup)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    if not all(line["ok"] for line in lines):
        sys.exit(1)


if __name__ == "__main__":
    main()
