"""The index kernels (kvcached_amd/csrc/index_kernels.hip) on a real MI355X at every seam of their launch geometry: the cases
and comparisons are tests/kvc_index_edges.py's, and tests/test_index_edges.py shows without a GPU that the cases reach the
seams and that the comparisons notice seven kinds of wrong kernel. Each sweep runs through both entries: the C ABI
(kvcached_amd.capi: a guarded output buffer, a NULL id pointer, `cap`) and the wrappers of integration/sglang/allocators.py
(which allocate `out` themselves: there only what the operation must write is compared). Bit for bit, every element.

Then one test per operation that the kernels run on torch's current stream, not on the default one.

Nothing here provokes a fault: every inconsistent input is one the kernels guard, and what a missing guard would show is a
sentinel overwritten or left in place inside a buffer this test owns."""
import numpy as np
import pytest
import torch

import kvc_index_edges as E
from kvc_index_edges import GUARD
from test_gpu_sglang_glue import DEV, dev, gpu_lib  # noqa: F401

pytestmark = pytest.mark.gpu

ENTRIES = pytest.mark.parametrize("entry", ["capi", "wrapper"])


# ------------------------------------------------------------------ the operations, as the sweeps take them
def _ids(capi, ids):
    """(pointer, count) of a host id list; no ids: a NULL pointer."""
    return (capi.i64_array(ids.tolist()), len(ids)) if len(ids) else (None, 0)


def _raw(call):
    """op(case, buf): upload the guarded buffer, let `call(case, address of the payload)` run on the default stream, read the
    whole buffer back."""
    def op(case, buf):
        d = torch.from_numpy(buf).to(DEV)
        call(case, d.data_ptr() + 8 * GUARD)
        torch.cuda.synchronize()
        return d.cpu().numpy()
    return op


def _wrapped(call):
    """op(case, buf): the wrapper's own output tensor, copied into the payload."""
    def op(case, buf):
        got = call(case)
        torch.cuda.synchronize()
        assert got.dtype == torch.int64 and got.device.type == "cuda" and got.numel() <= len(case["want"])
        buf[GUARD:GUARD + got.numel()] = got.cpu().numpy()
        return buf
    return op


def expand_op(capi, entry):
    from kvcached_amd.integration.sglang.allocators import expand_block_ids
    if entry == "wrapper":
        return _wrapped(lambda c: expand_block_ids(c["ids"].tolist(), c["tpb"], DEV))
    return _raw(lambda c, out: capi.check(capi.lib.kvc_expand_block_ids(*_ids(capi, c["ids"]), c["tpb"], out, None)))


def extend_op(capi, entry):
    from kvcached_amd.integration.sglang.allocators import alloc_extend_indices
    if entry == "wrapper":
        return _wrapped(lambda c: alloc_extend_indices(dev(c["prefix_lens"]), dev(c["seq_lens"]), dev(c["last_loc"]),
                                                       c["ids"].tolist(), c["tpb"], c["out_len"]))

    def call(c, out):
        pre, seq, loc = dev(c["prefix_lens"]), dev(c["seq_lens"]), dev(c["last_loc"])
        capi.check(capi.lib.kvc_alloc_extend_indices(pre.data_ptr(), seq.data_ptr(), loc.data_ptr(), len(c["seq_lens"]),
                                                     *_ids(capi, c["ids"]), c["tpb"], out, c["out_len"], None))
    return _raw(call)


def decode_op(capi, entry):
    from kvcached_amd.integration.sglang.allocators import alloc_decode_indices
    if entry == "wrapper":
        return _wrapped(lambda c: alloc_decode_indices(dev(c["seq_lens"]), dev(c["last_loc"]), c["ids"].tolist(), c["tpb"]))

    def call(c, out):
        seq, loc = dev(c["seq_lens"]), dev(c["last_loc"])
        capi.check(capi.lib.kvc_alloc_decode_indices(seq.data_ptr(), loc.data_ptr(), len(c["seq_lens"]), *_ids(capi, c["ids"]),
                                                     c["tpb"], out, None))
    return _raw(call)


def unique_op(capi, entry):
    from kvcached_amd.integration.sglang.allocators import unique_block_ids

    def uniq(idx, tpb, n_blocks):
        d = dev(idx)
        try:
            if entry == "wrapper":
                return unique_block_ids(d, tpb, n_blocks)
            return capi.unique_block_ids(d.data_ptr(), d.numel(), tpb, n_blocks)
        except RuntimeError as e:                          # (capi.KvcError is one)
            assert "outside" in str(e), e
            raise E.Refused(str(e))
    return uniq


# ------------------------------------------------------------------ the four sweeps
@ENTRIES
def test_expand_at_every_seam(gpu_lib, entry):
    """Totals on both sides of a multiple of 256 for nine block sizes, one id, none, and 1023 .. 2049 ids: the second and third
    launch of 1024 ids write at out + 1024 * tpb and out + 2048 * tpb. Nothing before `out`, nothing behind the total."""
    E.sweep_expand(expand_op(gpu_lib, entry), entry, "raw" if entry == "capi" else "written")


@ENTRIES
def test_extend_at_every_seam(gpu_lib, entry):
    """Requests of 0 .. 8193 tokens alone and between short and empty ones (token groups 1 and 2 of a request, workgroups that
    leave early), every phase of the prefix against blocks of 1 .. 5000 tokens with a block across a group seam, 1 .. 513
    requests, 0 / 1 / 1023 / 1024 / 1025 new blocks (NULL, kernarg, staged), totals of 4096 k and 4096 k + 1; an id list that is
    too short and an extend_num_tokens below the sum leave the sentinel exactly where nothing can be written."""
    E.sweep_extend(extend_op(gpu_lib, entry), entry, "raw" if entry == "capi" else "written")


@ENTRIES
def test_decode_at_every_seam(gpu_lib, entry):
    """1 .. 769 requests crossed with fifteen masks of which requests open a block: empty, partly and wholly block-opening
    waves and workgroups in front of, between and behind the others; 1023 / 1024 / 1025 new blocks; first tokens; an id list
    short by one."""
    E.sweep_decode(decode_op(gpu_lib, entry), entry, "raw" if entry == "capi" else "written")


@ENTRIES
@pytest.mark.parametrize("tpb", E.UNIQUE_TPBS)
def test_unique_over_every_word_range(gpu_lib, entry, tpb):
    """Touched bitmap words [lo, lo + len - 1] for lo around 0 and 1024 and len around 1, 1024 and 2048 (the sweep starts at lo
    and walks chunks of 1024 words from there), filled at the ends only, on both sides of every wave and chunk seam, wholly
    (every word full), and wholly with every third word empty."""
    E.run_unique(unique_op(gpu_lib, entry), E.unique_range_steps(tpb), E.Refused, entry)


@ENTRIES
def test_unique_growth_tails_and_hygiene(gpu_lib, entry):
    """In one context, from its first query on: the scratch bitmap at its minimum of 4096 words, one word more, 2^17 words and
    a small pool again; then 1 / 255 / 256 / 257 indices, 100000 indices into 3 blocks, pools of 64 / 65 / 95 blocks with the
    last block and the first index past it, and refused calls whose valid blocks must be in no later answer."""
    uniq = unique_op(gpu_lib, entry)
    E.run_unique(uniq, E.unique_growth_steps(), E.Refused, entry)
    for tpb in E.UNIQUE_TPBS:
        E.run_unique(uniq, E.unique_misc_steps(tpb), E.Refused, entry)


def test_unique_cap_through_the_c_abi(gpu_lib):
    """kvc_unique_block_ids with cap = count - 1 returns the count and leaves the host array alone; the next query is exact;
    cap = count fills exactly `count` elements."""
    capi = gpu_lib

    def raw(idx, tpb, n_blocks, host, cap):
        d = dev(idx)
        arr = (capi._i64 * len(host)).from_buffer(host)
        return capi.check(capi.lib.kvc_unique_block_ids(d.data_ptr(), d.numel(), tpb, n_blocks, arr, cap, None))

    E.check_unique_cap(raw, "capi")


# ------------------------------------------------------------------ stream order
@pytest.fixture(scope="module")
def big():
    t = torch.empty(1 << 30, dtype=torch.uint8, device=DEV)
    yield t
    del t
    torch.cuda.empty_cache()


def _pinned(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).pin_memory()


def _on_side_stream(big, device_inputs, real_inputs, call):
    """The device inputs hold a harmless decoy. On a side stream: several fills of 1 GiB, then the copy of the real inputs from
    pinned memory, then the operation, then the read of its result. An operation launched on any other stream runs while the
    fills are still going: it reads the decoy (a wrong answer, never a bad address)."""
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for i in range(8):
            big.fill_(i)
        for d, h in zip(device_inputs, real_inputs):
            d.copy_(h, non_blocking=True)
        got = call()
        if isinstance(got, torch.Tensor):
            got = got.cpu()                                 # on s: waits for s, and for s only
    s.synchronize()
    torch.cuda.synchronize()
    return got


def _case(cases, name):
    return next(c for c in cases if c["name"] == name)


def test_extend_runs_on_the_current_stream(gpu_lib, big):
    from kvcached_amd.integration.sglang.allocators import alloc_extend_indices
    c = _case(E.extend_cases(), "mixed_ext8193")
    assert len(c["ids"]) == len(c["free_pages"]) and c["out_len"] == len(c["want"])
    pre, seq, loc = dev(c["seq_lens"]), dev(c["seq_lens"]), dev(c["last_loc"])      # decoy: prefix == seq, nothing to write
    got = _on_side_stream(big, [pre, seq, loc], [_pinned(c[k]) for k in ("prefix_lens", "seq_lens", "last_loc")],
                          lambda: alloc_extend_indices(pre, seq, loc, c["ids"].tolist(), c["tpb"], c["out_len"]))
    assert np.array_equal(got.numpy(), c["want"])


def test_decode_runs_on_the_current_stream(gpu_lib, big):
    from kvcached_amd.integration.sglang.allocators import alloc_decode_indices
    c = _case(E.decode_cases(), "decode_bs513_alternating")
    seq, loc = dev(np.full(513, 2)), dev(np.zeros(513))                            # decoy: no request opens a block
    got = _on_side_stream(big, [seq, loc], [_pinned(c["seq_lens"]), _pinned(c["last_loc"])],
                          lambda: alloc_decode_indices(seq, loc, c["ids"].tolist(), c["tpb"]))
    assert np.array_equal(got.numpy(), c["want"])


def test_unique_runs_on_the_current_stream(gpu_lib, big):
    from kvcached_amd.integration.sglang.allocators import unique_block_ids
    step = E.unique_step("unique_on_a_side_stream", E.range_blocks(1025, 2049, "seams"), 16, (1025 + 2049) * 32)
    idx = dev(np.zeros(len(step["idx"])))                                          # decoy: every index 0
    got = _on_side_stream(big, [idx], [_pinned(step["idx"])], lambda: unique_block_ids(idx, 16, step["n_blocks"]))
    assert got == step["want"].tolist()
    # and the bitmap is clean for the next query, on the default stream
    assert unique_block_ids(dev([16 * 40000 + 3]), 16, step["n_blocks"]) == [40000]


def test_expand_runs_on_the_current_stream(gpu_lib, big):
    """expand has no device input, so the decoy is in its output: a tensor of the output's size is filled behind the 1 GiB fills
    and released, and the wrapper's torch.empty gets the same memory (asserted). Launched on any other stream the kernel would
    write first and the decoy fill would come down on its result. If the address differs, the caching allocator has changed its
    ways (a new torch, an allocator setting): that failure points at this test's premise, not at the kernel."""
    from kvcached_amd.integration.sglang.allocators import expand_block_ids
    c = _case(E.expand_cases(), "expand_n2049_t3")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for i in range(8):
            big.fill_(i)
        decoy = torch.empty(len(c["want"]), dtype=torch.int64, device=DEV)
        decoy.fill_(-1)
        address = decoy.data_ptr()
        del decoy
        out = expand_block_ids(c["ids"].tolist(), c["tpb"], DEV)
        assert out.data_ptr() == address, "torch.empty did not reuse the decoy's memory: the premise of this test, not the kernel"
        got = out.cpu()
    s.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(got.numpy(), c["want"])
