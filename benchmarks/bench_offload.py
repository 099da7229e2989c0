"""Offload / restore of live KV blocks to pinned host memory (KVCacheManager.offload / .restore, HIP kernels
copy_blocks_to_host / copy_blocks_from_host) against the host link itself and a torch formulation.

One JSON line per geometry and size. Geometries: Llama-3-8B (32 layers, K/V, 16 tokens x 2 KiB cells = 32 KiB blocks)
in the non-contiguous layout (64 regions) and in the contiguous one (1 region, 2 MiB per block); n = 8, 64, 512 blocks
(512 blocks = 1 GiB). Per line:
  offload_copy_ms / restore_copy_ms  device events around the kernel launches alone (median of --steps)
  offload_call_ms                    host clock around offload() (copy, wait, free())
  restore_call_ms                    host clock around restore() (alloc(), copy) and a synchronise
  link_d2h_GBps / link_h2d_GBps      the link ceiling in the same process: one contiguous device tensor of the same size
                                     copied to / from a pinned tensor with copy_(non_blocking=True)
  torch_d2h_ms                       per region index_select of the blocks, then a copy to pinned memory
  torch_h2d_ms                       per region a copy from pinned memory, then index_copy_ into the blocks
  bit_exact                          seeded blocks -> offload image == torch's gather, and restore puts them back

Usage: python benchmarks/bench_offload.py [--steps 10] [--warmup 3] [--sizes 8,64,512] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("KVCACHED_PAGE_PREALLOC_ENABLED", "false")
os.environ.setdefault("KVCACHED_IPC_NAME", f"kvc_bench_offload_{os.getpid()}")
os.environ.setdefault("KVCACHED_LOG_LEVEL", "ERROR")

import torch  # noqa: E402

PAGE = 2 << 20
DEV = "cuda:0"
LAYERS, BLOCK_TOKENS, CELL = 32, 16, 2048


def _event_ms(fn, steps, warmup):
    """Median device time of fn() on the current stream, bracketed by events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


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
    # a stream of our own: its handle is what the kernels are launched on (in the C ABI, NULL names the library's stream)
    st = torch.cuda.Stream()
    stream = st.cuda_stream
    lines = []
    try:
        for n in sizes:
            with torch.cuda.stream(st):
                nbytes = n * R * bb
                ids = m.alloc(n)
                g = torch.Generator(device=DEV).manual_seed(n)
                ids_t = torch.tensor(ids, device=DEV)
                for v in views:
                    v[ids_t] = torch.randint(0, 256, (n, bb), dtype=torch.uint8, device=DEV, generator=g)
                torch.cuda.synchronize()
                host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
                # the kernels alone, on the same blocks
                d2h = _event_ms(lambda: capi.copy_blocks_to_host(0, ids, bb, host.data_ptr(), stream, sync=False), steps, warmup)
                # torch: per region gather, then a copy to pinned memory (region-major image)
                tbuf = torch.empty((R, n, bb), dtype=torch.uint8, pin_memory=True)

                def torch_d2h():
                    for r, v in enumerate(views):
                        tbuf[r].copy_(v.index_select(0, ids_t), non_blocking=True)
                t_d2h = _event_ms(torch_d2h, steps, warmup)
                torch.cuda.synchronize()
                exact = torch.equal(host.view(n, R, bb).transpose(0, 1), tbuf)
                want = tbuf.to(DEV)

                def torch_h2d():   # the way back: per region a copy from pinned memory, then index_copy_ into the blocks
                    for r, v in enumerate(views):
                        v.index_copy_(0, ids_t, tbuf[r].to(DEV, non_blocking=True))
                t_h2d = _event_ms(torch_h2d, steps, warmup)
                # the link ceiling: one contiguous tensor of the same size, each direction
                dev = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
                pin = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
                link_d2h = _event_ms(lambda: pin.copy_(dev, non_blocking=True), steps, warmup)
                link_h2d = _event_ms(lambda: dev.copy_(pin, non_blocking=True), steps, warmup)
                del dev, pin
                # whole calls: offload (copy, wait, free) and restore (alloc, copy, synchronise)
                call_off, call_res, copy_res = [], [], []
                for i in range(warmup + steps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    h = m.offload(ids, out=host)
                    t1 = time.perf_counter()
                    new = m.restore(h)
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    # the restore kernel alone, into the blocks it just filled
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    capi.copy_blocks_from_host(0, new, bb, host.data_ptr(), stream, sync=False)
                    b.record()
                    b.synchronize()
                    if i >= warmup:
                        call_off.append((t1 - t0) * 1e3)
                        call_res.append((t2 - t1) * 1e3)
                        copy_res.append(a.elapsed_time(b))
                    h.release()
                    new_t = torch.tensor(new, device=DEV)
                    for r, v in enumerate(views):
                        exact = exact and torch.equal(v[new_t], want[r])
                    ids, ids_t = new, new_t
                h2d = statistics.median(copy_res)
                gbps = lambda ms: round(nbytes / ms / 1e6, 2)   # noqa: E731
                line = {
                    "bench": "offload", "layout": "contiguous" if contiguous else "per_layer", "regions": R,
                    "block_bytes": bb, "n_blocks": n, "bytes": nbytes,
                    "offload_copy_ms": round(d2h, 4), "offload_copy_GBps": gbps(d2h),
                    "restore_copy_ms": round(h2d, 4), "restore_copy_GBps": gbps(h2d),
                    "offload_call_ms": round(statistics.median(call_off), 4),
                    "restore_call_ms": round(statistics.median(call_res), 4),
                    "link_d2h_ms": round(link_d2h, 4), "link_d2h_GBps": gbps(link_d2h),
                    "link_h2d_ms": round(link_h2d, 4), "link_h2d_GBps": gbps(link_h2d),
                    "offload_vs_link_d2h": round(link_d2h / d2h, 3), "restore_vs_link_h2d": round(link_h2d / h2d, 3),
                    "torch_d2h_ms": round(t_d2h, 4), "torch_d2h_GBps": gbps(t_d2h),
                    "torch_h2d_ms": round(t_h2d, 4), "torch_h2d_GBps": gbps(t_h2d),
                    "bit_exact": bool(exact), "steps": steps, "warmup": warmup,
                }
                print(json.dumps(line), flush=True)
                lines.append(line)
                m.free(ids)
                del host, tbuf, want
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
    assert torch.cuda.is_available(), "bench_offload needs the MI355X"
    sizes = [int(s) for s in a.sizes.split(",")]
    lines = []
    for layout in a.layouts.split(","):
        lines += run_geometry(layout == "contiguous", sizes, a.steps, a.warmup)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    if not all(line["bit_exact"] for line in lines):
        sys.exit(1)


if __name__ == "__main__":
    main()
