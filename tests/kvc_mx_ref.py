"""CPU restatement of the MXFP8 host image of KV blocks, written from the format's definition and the
OCP Microscaling specification, not from the kernel: what tests/test_kv_codec.py pins and tests/test_gpu_kv_codec.py
compares the encode / decode kernels against, bit for bit.

A group is 32 consecutive 16-bit floats. Its shared exponent se is the smallest integer with amax * 2^-se <= 448 (the
largest e4m3fn value), clamped to [-127, 127], -127 for an all-zero group; the scale byte is se + 127 (E8M0); the code of
an element v is v * 2^-se rounded to e4m3fn, to nearest even. A group that holds a NaN or an infinity has the scale byte
0xFF and 32 zero codes, and decodes to 32 canonical quiet NaNs. A NaN code (0x7F or 0xFF) under a scale byte other than
0xFF is never written by the encoder and decodes to a NaN of unspecified sign and payload. (tests/kvc_mx_exact.py states
the same format in exact float64 arithmetic; tests/test_kv_codec.py holds the two against each other on every input.)"""
import torch

GROUP = 32
QUIET_NAN = {torch.bfloat16: 0x7FC0, torch.float16: 0x7E00}
CODEC = {torch.bfloat16: 1, torch.float16: 2}       # KVC_CODEC_MXFP8_BF16 / _F16


def record_bytes(block_bytes):
    return block_bytes // 2 + block_bytes // 64


def encode(v16):
    """bf16 / fp16 tensor, numel % 32 == 0 -> (codes uint8 [groups, 32], scale bytes uint8 [groups])."""
    v = v16.float().reshape(-1, GROUP)
    bad = ~torch.isfinite(v).all(1)
    v = torch.where(bad[:, None], torch.zeros_like(v), v)
    amax = v.abs().amax(1)
    m, ex = torch.frexp(amax)                        # amax = m * 2^ex, m in [0.5, 1)
    e = ex - 1
    se = torch.where(m * 2 <= 1.75, e - 8, e - 7)
    se = torch.where(amax == 0, torch.full_like(se, -127), se).clamp(-127, 127)
    codes = torch.ldexp(v, (-se)[:, None].expand_as(v)).to(torch.float8_e4m3fn).view(torch.uint8)
    scales = (se + 127).to(torch.uint8)
    scales[bad] = 0xFF                               # rule 4 (the codes of such a group are already zero)
    return codes, scales


def decode(codes, scales, dt):
    """(codes [groups, 32], scale bytes [groups]) -> flat tensor of dtype dt."""
    q = codes.view(torch.float8_e4m3fn).float()
    se = scales.int() - 127
    out = torch.ldexp(q, se[:, None].expand_as(q)).to(dt)
    out[scales == 0xFF] = torch.tensor([QUIET_NAN[dt]], dtype=torch.int16).view(dt)   # rule 4, whatever the codes are
    return out.reshape(-1)


def shared_exponents(scales):
    return scales.int() - 127


def encode_block(v16):
    """One (block, region) record: the codes in element order, then the scale bytes in group order (uint8, flat)."""
    codes, scales = encode(v16.reshape(-1))
    return torch.cat([codes.reshape(-1), scales])


def decode_block(record, dt):
    """A flat uint8 record (the codes, then one scale byte per 32 of them) -> its elements, of dtype dt."""
    groups = record.numel() // (GROUP + 1)
    return decode(record[:groups * GROUP].reshape(groups, GROUP), record[groups * GROUP:], dt)
