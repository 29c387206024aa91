"""Pure-PyTorch reference implementations of the engine's hot ops.

These are the numerics oracle for the HIP/CDNA4 kernels (tests compare the
HIP kernel against these in fp32 — SURVEY.md §4 test strategy (c)) and the
CPU execution path. They are intentionally simple and readable; the GPU path
never runs these (opsagent_amd.ops dispatch raises if the HIP extension is
missing on a GPU box).
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch


def _acc(x: torch.Tensor) -> torch.Tensor:
    """Working precision: fp32, or fp64 for an fp64 input (a model built in
    fp64 is then fp64 throughout, which the whole-model oracle test uses)."""
    return x if x.dtype == torch.float64 else x.float()


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    dtype = x.dtype
    xf = _acc(x)
    var = xf.pow(2).mean(dim=-1, keepdim=True)
    out = xf * torch.rsqrt(var + eps) * weight.to(xf.dtype)
    return out.to(dtype)


def fused_add_rms_norm(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Returns (rmsnorm(x + residual), x + residual)."""
    s = (_acc(x) + _acc(residual))
    out = rms_norm(s, weight, eps)
    return out.to(x.dtype), s.to(x.dtype)


def rope_cos_sin(
    max_seq: int, head_dim: int, theta: float = 500000.0, device="cpu", dtype=torch.float32
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Precomputed RoPE tables [max_seq, head_dim/2] (host-side per CDNA guide §B)."""
    inv_freq = 1.0 / (
        theta ** (torch.arange(0, head_dim, 2, device=device, dtype=torch.float32) / head_dim)
    )
    t = torch.arange(max_seq, device=device, dtype=torch.float32)
    freqs = torch.outer(t, inv_freq)
    return freqs.cos().to(dtype), freqs.sin().to(dtype)


def rope_apply(
    q: torch.Tensor,
    k: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
    positions: torch.Tensor,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Neox-style (rotate-half) RoPE.

    q: [T, Hq, D], k: [T, Hk, D]; cos/sin: [max_seq, D/2]; positions: [T].
    """
    def _rot(x: torch.Tensor) -> torch.Tensor:
        d = x.shape[-1]
        x1 = _acc(x[..., : d // 2])
        x2 = _acc(x[..., d // 2 :])
        c = cos[positions].to(x1.dtype).unsqueeze(1)  # [T,1,D/2]
        s = sin[positions].to(x1.dtype).unsqueeze(1)
        return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(x.dtype)

    return _rot(q), _rot(k)


def silu_mul(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    return (torch.nn.functional.silu(_acc(gate)) * _acc(up)).to(gate.dtype)


def attention_prefill(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    scale: Optional[float] = None,
    causal: bool = True,
) -> torch.Tensor:
    """Causal attention over contiguous tensors.

    q: [B, Hq, Sq, D]; k, v: [B, Hk, Skv, D] with Skv >= Sq (the causal
    diagonal is offset so that query i attends keys [0 .. Skv-Sq+i]).
    GQA: Hq % Hk == 0 (kv heads broadcast over query-head groups).
    """
    B, Hq, Sq, D = q.shape
    Hk, Skv = k.shape[1], k.shape[2]
    scale = scale if scale is not None else D ** -0.5
    group = Hq // Hk
    kf = _acc(k).repeat_interleave(group, dim=1)
    vf = _acc(v).repeat_interleave(group, dim=1)
    s = torch.einsum("bhqd,bhkd->bhqk", _acc(q), kf) * scale
    if causal:
        offset = Skv - Sq
        qi = torch.arange(Sq, device=q.device).unsqueeze(1)
        ki = torch.arange(Skv, device=q.device).unsqueeze(0)
        mask = ki > (qi + offset)
        s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    out = torch.einsum("bhqk,bhkd->bhqd", p, vf)
    return out.to(q.dtype)


def attention_decode_paged(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_table: torch.Tensor,
    seq_lens: torch.Tensor,
    scale: Optional[float] = None,
) -> torch.Tensor:
    """Single-token decode attention against a paged KV cache.

    q:           [B, Hq, D]         (one new token per sequence)
    k/v_cache:   [num_blocks, block_size, Hk, D]
    block_table: [B, max_blocks] int32 (block ids per sequence, -1 padded)
    seq_lens:    [B] int32 — total tokens in cache per sequence (incl. current)
    """
    B, Hq, D = q.shape
    block_size = k_cache.shape[1]
    Hk = k_cache.shape[2]
    group = Hq // Hk
    scale = scale if scale is not None else D ** -0.5
    outs = []
    for b in range(B):
        n = int(seq_lens[b].item())
        nblocks = (n + block_size - 1) // block_size
        blocks = block_table[b, :nblocks].long()
        k = _acc(k_cache[blocks].reshape(-1, Hk, D)[:n])  # [n, Hk, D]
        v = _acc(v_cache[blocks].reshape(-1, Hk, D)[:n])
        kf = k.repeat_interleave(group, dim=1)  # [n, Hq, D]
        vf = v.repeat_interleave(group, dim=1)
        s = torch.einsum("hd,nhd->hn", _acc(q[b]), kf) * scale
        p = torch.softmax(s, dim=-1)
        outs.append(torch.einsum("hn,nhd->hd", p, vf))
    return torch.stack(outs).to(q.dtype)


def attention_append_paged(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_table: torch.Tensor,
    seq_lens: torch.Tensor,
    cu_q: torch.Tensor,
    scale: Optional[float] = None,
) -> torch.Tensor:
    """Append attention: sequence b has L_b = cu_q[b+1]-cu_q[b] new query
    tokens whose K/V are already in the cache; seq_lens[b] counts all keys
    including them. Token j is decode attention at length seq_lens[b]-L_b+j+1.

    q: [T, Hq, D]; returns [T, Hq, D].
    """
    B = seq_lens.shape[0]
    outs = []
    for b in range(B):
        t0, t1 = int(cu_q[b].item()), int(cu_q[b + 1].item())
        n, L = int(seq_lens[b].item()), t1 - t0
        for j in range(L):
            length = torch.tensor([n - L + j + 1], dtype=seq_lens.dtype, device=seq_lens.device)
            outs.append(
                attention_decode_paged(
                    q[t0 + j : t0 + j + 1], k_cache, v_cache, block_table[b : b + 1], length, scale
                )
            )
    return torch.cat(outs, dim=0)


def kv_cache_write(
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    slot_mapping: torch.Tensor,
) -> None:
    """Scatter new K/V rows into the paged cache.

    k/v: [T, Hk, D]; slot_mapping: [T] int64 flat slot = block_id*block_size + offset.
    """
    nb, bs, hk, d = k_cache.shape
    k_cache.view(nb * bs, hk, d)[slot_mapping] = k
    v_cache.view(nb * bs, hk, d)[slot_mapping] = v


def quant_fp8(x: torch.Tensor):
    """Per-row OCP e4m3 quantization reference (torch.float8_e4m3fn)."""
    shape = x.shape
    xf = x.reshape(-1, shape[-1]).float()
    amax = xf.abs().amax(dim=-1, keepdim=True).clamp_min(1e-8)
    scale = (amax / 448.0).squeeze(-1)
    q = (xf / scale.unsqueeze(-1)).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).reshape(shape), scale


def dequant_fp8(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    f = q.view(torch.float8_e4m3fn).float()
    return f * scale.unsqueeze(-1)


def rope_kv_fp8(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    k_codes: torch.Tensor,
    v_codes: torch.Tensor,
    k_scale: torch.Tensor,
    v_scale: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
    positions: torch.Tensor,
    slot_mapping: torch.Tensor,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """RoPE(q, k), then quantise roped k and v per (token, head) row and
    scatter codes + scales into the fp8 paged cache.

    codes: uint8 [num_blocks, block_size, Hk, D]; scales: f32 [num_blocks,
    block_size, Hk]. Returns (roped q, roped k, v)."""
    q2, k2 = rope_apply(q, k, cos, sin, positions)
    nb, bs, hk, d = k_codes.shape
    slots = slot_mapping.long()
    for x, codes, scales in ((k2, k_codes, k_scale), (v, v_codes, v_scale)):
        c, s = quant_fp8(x)                       # [T, Hk, D], [T*Hk]
        codes.view(nb * bs, hk, d)[slots] = c
        scales.view(nb * bs, hk)[slots] = s.view(-1, hk)
    return q2, k2, v


def kv_gather_fp8(
    k_codes: torch.Tensor,
    v_codes: torch.Tensor,
    k_scale: torch.Tensor,
    v_scale: torch.Tensor,
    slots: torch.Tensor,
    dtype: torch.dtype = torch.bfloat16,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Gather + dequantise: [Skv, Hk, D] K and V with value
    dtype(float(code) * scale) for the given flat slots."""
    nb, bs, hk, d = k_codes.shape
    idx = slots.long()
    outs = []
    for codes, scales in ((k_codes, k_scale), (v_codes, v_scale)):
        c = codes.view(nb * bs, hk, d)[idx]
        s = scales.view(nb * bs, hk)[idx]
        outs.append(dequant_fp8(c, s).to(dtype))
    return outs[0], outs[1]


def attention_decode_paged_fp8(
    q: torch.Tensor,
    k_codes: torch.Tensor,
    v_codes: torch.Tensor,
    k_scale: torch.Tensor,
    v_scale: torch.Tensor,
    block_table: torch.Tensor,
    seq_lens: torch.Tensor,
    scale: Optional[float] = None,
) -> torch.Tensor:
    """Decode attention over the fp8 paged cache: dequantise, then the
    reference paged attention."""
    kc = dequant_fp8(k_codes, k_scale)
    vc = dequant_fp8(v_codes, v_scale)
    return attention_decode_paged(q, kc, vc, block_table, seq_lens, scale)


def attention_append_paged_fp8(
    q: torch.Tensor,
    k_codes: torch.Tensor,
    v_codes: torch.Tensor,
    k_scale: torch.Tensor,
    v_scale: torch.Tensor,
    block_table: torch.Tensor,
    seq_lens: torch.Tensor,
    cu_q: torch.Tensor,
    scale: Optional[float] = None,
) -> torch.Tensor:
    """Append attention over the fp8 paged cache: dequantise, then the
    reference append attention."""
    kc = dequant_fp8(k_codes, k_scale)
    vc = dequant_fp8(v_codes, v_scale)
    return attention_append_paged(q, kc, vc, block_table, seq_lens, cu_q, scale)


def linear_fp8(x: torch.Tensor, w8: torch.Tensor, w_scale: torch.Tensor) -> torch.Tensor:
    w = dequant_fp8(w8, w_scale)
    return torch.nn.functional.linear(x.float(), w).to(x.dtype)


def greedy_sample_masked(logits: torch.Tensor, mask: Optional[torch.Tensor]) -> torch.Tensor:
    """argmax over allowed tokens. logits [B, V]; mask [B, V] bool (True = allowed).
    The largest by IEEE comparison (-0 equals +0), the lowest index among
    equals, -1 where no allowed logit is > -inf, as the kernel gives."""
    lf = logits.float()
    if mask is not None:
        lf = lf.masked_fill(~mask, float("-inf"))
    tok = lf.argmax(dim=-1)
    return torch.where((lf > float("-inf")).any(dim=-1), tok, torch.full_like(tok, -1))


def head_argmax(
    x: torch.Tensor, w: torch.Tensor, mask: Optional[torch.Tensor]
) -> torch.Tensor:
    """Greedy decode head: linear, rounded to bf16 as the logits row is, then
    the masked greedy pick. x [M, K]; w [V, K]; mask [M, V] bool or None.
    Returns int64 [M], -1 where no allowed logit is > -inf."""
    logits = torch.nn.functional.linear(x, w).to(torch.bfloat16)
    return greedy_sample_masked(logits, mask)


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 on numpy uint32 counter arrays; returns four uint32
    arrays. Integer arithmetic only (64-bit products, masked)."""
    import numpy as np

    M = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M for c in (c0, c1, c2, c3))
    k0 = np.uint64(k0 & 0xFFFFFFFF)
    k1 = np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (
            (p1 >> np.uint64(32)) ^ c1 ^ k0,
            p1 & M,
            (p0 >> np.uint64(32)) ^ c3 ^ k1,
            p0 & M,
        )
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def sample_masked(
    logits: torch.Tensor,
    mask: Optional[torch.Tensor],
    inv_temp: torch.Tensor,
    top_k: torch.Tensor,
    top_p: torch.Tensor,
    seed: torch.Tensor,
    step: torch.Tensor,
    adj: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None,
    info: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Seeded sampler, the twin of sample.hip: mask first, then sparse
    adjustments, top-k by value, top-p by value level, Gumbel-max draw with
    Philox noise keyed by (seed, step, token). fp32 where the kernel is fp32,
    top-p masses as w * 2^40 integers. logits [B, V]; mask [B, V] bool or
    None; inv_temp f32, top_k i32, top_p f32, seed/step int64 (the u64 bits)
    [B]; adj = (adj_ptr i32 [B+1], adj_tok i32 [nnz], adj_val f32 [nnz]),
    tokens sorted and unique per row. Returns int64 [B], -1 where no
    candidate exists; fills info int32 [B, 2] (kept count, bits of the
    smallest kept z) when given."""
    import numpy as np

    B, V = logits.shape
    x = logits.detach().float().cpu().numpy()
    m = None if mask is None else mask.detach().cpu().numpy().astype(bool)
    it_a = inv_temp.detach().cpu().numpy().astype(np.float32)
    k_a = top_k.detach().cpu().numpy().astype(np.int64)
    p_a = top_p.detach().cpu().numpy().astype(np.float32)
    seed_a = seed.detach().cpu().numpy().astype(np.int64).view(np.uint64)
    step_a = step.detach().cpu().numpy().astype(np.int64).view(np.uint64)
    if adj is not None:
        aptr = adj[0].detach().cpu().numpy()
        atok = adj[1].detach().cpu().numpy()
        aval = adj[2].detach().cpu().numpy().astype(np.float32)
    out = np.full(B, -1, dtype=np.int64)
    inf_bits = 0x7F800000
    info_np = np.zeros((B, 2), dtype=np.int32)
    info_np[:, 1] = inf_bits
    for b in range(B):
        z = x[b].copy()
        if adj is not None:
            a0, a1 = int(aptr[b]), int(aptr[b + 1])
            ok = (atok[a0:a1] >= 0) & (atok[a0:a1] < V)
            t = atok[a0:a1][ok]
            z[t] = z[t] + aval[a0:a1][ok]  # one fp32 add
        with np.errstate(invalid="ignore"):
            cand = z > -np.inf  # false for NaN
        if m is not None:
            cand &= m[b]
        ncand = int(cand.sum())
        if ncand == 0:
            continue
        it, k, p = it_a[b], int(k_a[b]), p_a[b]
        zc = np.where(cand, z, -np.inf).astype(np.float32)
        if not it > 0:
            win = int(np.argmax(zc))
            out[b] = win
            # the kernel's key holds z + 0: a winning -0 is reported as +0
            info_np[b] = (ncand, int((z[win : win + 1] + np.float32(0)).view(np.int32)[0]))
            continue
        keep = cand.copy()
        zmax = zc.max()
        if 0 < k < ncand:
            tau = np.partition(zc, V - k)[V - k]
            keep &= zc >= tau
        if p < 1.0:
            idx = np.nonzero(keep)[0]
            zk = zc[idx]
            s = (zk * it).astype(np.float32)
            smax = np.float32(zmax * it)
            w = np.exp((s - smax).astype(np.float32)).astype(np.float32)
            wfix = np.rint(w.astype(np.float64) * 2.0**40).astype(np.int64)
            lev, inv = np.unique(zk, return_inverse=True)  # ascending
            mass = np.zeros(lev.shape[0], dtype=np.int64)
            np.add.at(mass, inv, wfix)
            Z = int(mass.sum())
            limit = int(float(p) * float(Z)) if p > 0 else 0
            above = Z - np.cumsum(mass)  # mass strictly above each level
            ok = (above <= limit) & (mass > 0)
            tau = lev[np.nonzero(ok)[0][0]]
            keep &= zc >= tau
        idx = np.nonzero(keep)[0]
        sd, st = int(seed_a[b]), int(step_a[b])
        words = philox4x32_10(
            idx >> 2, st & 0xFFFFFFFF, st >> 32, 0, sd & 0xFFFFFFFF, sd >> 32
        )
        r = np.choose(idx & 3, words)
        u = ((2 * (r >> 9) + 1).astype(np.float32) * np.float32(2.0**-24)).astype(np.float32)
        g = (-np.log(-np.log(u))).astype(np.float32)
        key = ((zc[idx] * it).astype(np.float32) + g).astype(np.float32)
        out[b] = int(idx[int(np.argmax(key))])
        info_np[b] = (idx.shape[0], int(zc[idx].min(keepdims=True).view(np.int32)[0]))
    if info is not None:
        info.copy_(torch.from_numpy(info_np).to(info.device))
    return torch.from_numpy(out)
