"""Whole-model fp64 oracle, bf16 emulation, mutants, a row recorder for a
live engine and the scenarios that drive every forward path. No pytest
dependency; see docs/KERNELS.md, "Verification method".

The oracle computes a set of ENTRIES at once. An entry is one token at one
RoPE position; `count[i, j]` says how often entry i attends the K/V of
entry j, `zeros[i]` how many all-zero cache slots it attends besides. A
plain sequence is the lower triangle; several sequences, a rejected
speculative branch or a wrong block table are other matrices over the same
entries, which is how the mutants are written.
"""

from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from attention_oracle import MUTANT_FACTOR, TOL_FACTOR, row_rel_err  # noqa: F401 (re-exported)

GAIN = 1.25      # q and k rows of qkv_w (1.5 gave the same ranking at smaller margins)
THETA = 32.0     # RoPE base: every pair turns visibly within 100 positions
BLOCK = 32


# --------------------------------------------------------------------------
# constructed model
# --------------------------------------------------------------------------
@torch.no_grad()
def construct_model_(model, seed: int = 2024, gain: float = GAIN, theta: float = THETA):
    """Overwrite a built LlamaForCausalLM in place (before its first forward):
    q/k gain, signed per-element norm weights (final norm included), RoPE
    tables of a small theta. Norm weights are bf16 values whatever the
    model's dtype; the tables are fp32."""
    from opsagent_amd import ops

    gen = torch.Generator().manual_seed(seed)
    h = model.spec.hidden_size

    def norm_w(p):
        mag = 0.5 + torch.rand(h, generator=gen)
        sign = torch.where(torch.rand(h, generator=gen) < 0.5, -1.0, 1.0)
        w = (mag * sign).to(torch.bfloat16)
        p.data.copy_(w.to(p.dtype))

    for layer in model.layers:
        at = layer.attn
        nqk = (at.hq + at.hk) * at.hd
        w = at.qkv_w.data
        w[:nqk] = (w[:nqk].double() * gain).to(w.dtype)
        norm_w(layer.input_norm_w)
        norm_w(layer.post_norm_w)
    norm_w(model.final_norm_w)
    cos, sin = ops.rope_cos_sin(model.spec.max_seq_len, model.spec.head_dim, theta)
    model.rope_cos.copy_(cos.to(model.rope_cos.device))
    model.rope_sin.copy_(sin.to(model.rope_sin.device))
    return model


def weights_of(model) -> dict:
    """The raw weight tensors as fp64 on the CPU (exact for bf16/fp32)."""
    def c(t):
        return t.detach().to("cpu", torch.float64)

    at0 = model.layers[0].attn
    return dict(
        embed=c(model.embed), lm_head=c(model.lm_head), final_w=c(model.final_norm_w),
        cos=c(model.rope_cos), sin=c(model.rope_sin), eps=float(model.spec.rms_eps),
        hq=at0.hq, hk=at0.hk, hd=at0.hd, inter=model.layers[0].mlp.i_local,
        layers=[
            dict(in_w=c(l.input_norm_w), post_w=c(l.post_norm_w), qkv=c(l.attn.qkv_w),
                 o=c(l.attn.o_w), gate_up=c(l.mlp.gate_up_w), down=c(l.mlp.down_w))
            for l in model.layers
        ],
    )


# --------------------------------------------------------------------------
# entries
# --------------------------------------------------------------------------
class Script:
    """Entries plus who attends whom. `add` appends a token run that
    continues `parent` (a chain: entry index per position) after its first
    `fork` positions and returns the new chain."""

    def __init__(self):
        self.tok: List[int] = []
        self.pos: List[int] = []
        self.keys: List[List[int]] = []

    def add(self, tokens: Sequence[int], parent: Optional[List[int]] = None,
            fork: int = 0) -> List[int]:
        chain = list(parent[:fork]) if parent is not None else []
        assert len(chain) == fork
        for t in tokens:
            i = len(self.tok)
            self.tok.append(int(t))
            self.pos.append(len(chain))
            chain.append(i)
            self.keys.append(list(chain))
        return chain

    def __len__(self):
        return len(self.tok)

    def count(self) -> torch.Tensor:
        n = len(self)
        c = torch.zeros(n, n, dtype=torch.float64)
        for i, ks in enumerate(self.keys):
            for j in ks:
                c[i, j] += 1
        return c

    def positions(self) -> torch.Tensor:
        return torch.tensor(self.pos, dtype=torch.long)


# --------------------------------------------------------------------------
# oracle / emulation
# --------------------------------------------------------------------------
def _bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


def forward(W: dict, tokens, pos=None, count=None, zeros=None, *, dtype=torch.float64,
            rnd: bool = False, rows=None, no_resid_attn=False, resid_twice=False,
            head_shift=False, k_unroped=False, kv_prev_layer=False,
            want_logits=True, forced=None, gathered=None, alt=None, device=None,
            want_kv=False):
    """fp64 forward of the entries (dtype/rnd give the emulations: fp32, and
    fp32 with a bf16 rounding wherever a correct GPU path stores bf16).
    Returns (final-norm hidden [T, H], logits [T, V]).

    Mutant knobs act on the entries `rows` (default all): residual not
    updated after attention, residual added twice behind the o projection,
    q-head h on kv-head (h+1)//G, cached K read un-roped, cached K/V of the
    layer below. "Cached" is every key but the entry's own.

    The fp8 cache (tests/model_fp8_cases.py): `forced` is a per-layer list of
    (K, V) [T, Hk, D] that every entry attends in place of the computed k and
    v, its own key included; `gathered` marks the rows that read those values
    rounded to bf16 (the prefill gather; emulation only); `alt` = (mask
    [T, T], kv) reads the pairs (row, key) of the mask from kv[layer], or from
    the entries' own unquantised k and v where kv is None; `device(layer, k,
    v, k_raw)` returns the (K, V) a simulated cache gives back. With want_kv
    the entries' own roped k and v per layer are returned as a third value."""
    r = _bf16 if rnd else (lambda x: x)
    tok = torch.as_tensor(list(tokens), dtype=torch.long)
    T = tok.numel()
    pos = torch.arange(T) if pos is None else torch.as_tensor(pos, dtype=torch.long)
    count = torch.tril(torch.ones(T, T)) if count is None else count
    count = count.to(dtype)
    zeros = torch.zeros(T) if zeros is None else torch.as_tensor(zeros)
    zeros = zeros.to(dtype)
    rows = torch.ones(T, dtype=torch.bool) if rows is None else rows
    hq, hk, hd = W["hq"], W["hk"], W["hd"]
    G = hq // hk
    eps = W["eps"]
    half = hd // 2
    cos = W["cos"][pos].to(dtype)[:, None, :]
    sin = W["sin"][pos].to(dtype)[:, None, :]
    kvh = torch.tensor([((h + 1) // G) % hk if head_shift else h // G for h in range(hq)])
    kvh_true = torch.tensor([h // G for h in range(hq)])
    eye = torch.eye(T, dtype=torch.bool)
    scale = hd ** -0.5

    def norm(x, w):
        return x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + eps) * w.to(dtype)

    def rope(x):
        x1, x2 = x[..., :half], x[..., half:]
        return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)

    resid = W["embed"][tok].to(dtype)
    pend = torch.zeros_like(resid)       # MLP output awaiting the fused add
    prev_kv = None
    own = []                             # per layer: the entries' own roped k and v
    for L in W["layers"]:
        s0 = resid + pend                # the norm reads the unrounded sum
        h = r(norm(s0, L["in_w"]))
        resid = r(s0)
        qkv = r(h @ L["qkv"].to(dtype).T)
        q = qkv[:, : hq * hd].reshape(T, hq, hd)
        k_raw = qkv[:, hq * hd: (hq + hk) * hd].reshape(T, hk, hd)
        v = qkv[:, (hq + hk) * hd:].reshape(T, hk, hd)
        q, k = r(rope(q)), r(rope(k_raw))
        k_own, v_own = k, v
        own.append((k_own, v_own))
        if device is not None:
            k, v = device(len(own) - 1, k, v, k_raw)
        if forced is not None:
            k, v = (t.to(dtype) for t in forced[len(own) - 1])
        qh = q.permute(1, 0, 2)                                   # [hq, T, D]

        def scores(K, hmap):
            return (qh @ K[:, hmap].permute(1, 2, 0)) * scale    # [hq, T, T]

        s = scores(k, kvh_true)
        if head_shift:
            s = torch.where(rows[None, :, None], scores(k, kvh), s)
        Kc = Vc = None
        if k_unroped:
            Kc, Vc = k_raw, v
        if kv_prev_layer and prev_kv is not None:
            Kc, Vc = prev_kv
        cached = (rows[:, None] & ~eye)[None]                     # [1, T, T]
        if alt is not None:
            cached = alt[0][None]
            Kc, Vc = (k_own, v_own) if alt[1] is None else (
                t.to(dtype) for t in alt[1][len(own) - 1])
        if Kc is not None:
            s = torch.where(cached, scores(Kc, kvh_true), s)
        if gathered is not None and rnd:
            assert Kc is None and not head_shift
            s = torch.where(gathered[None, :, None], scores(_bf16(k), kvh_true), s)
        live = (count > 0)[None]
        s = torch.where(live, s, torch.full_like(s, float("-inf")))
        m = s.amax(dim=-1, keepdim=True)
        m = torch.where(zeros[None, :, None] > 0, m.clamp_min(0.0), m)
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        p = count[None] * torch.exp(s - m)
        l = p.sum(dim=-1, keepdim=True) + zeros[None, :, None] * torch.exp(-m)
        p = r(p)

        def pv(P, V, hm):
            return P @ V[:, hm].permute(1, 0, 2)                  # [hq, T, D]

        if Kc is not None:
            pc = p * cached
            o = pv(p - pc, v, kvh_true) + pv(pc, Vc, kvh_true)
        elif head_shift:
            o = torch.where(rows[None, :, None], pv(p, v, kvh), pv(p, v, kvh_true))
        elif gathered is not None and rnd:
            o = torch.where(gathered[None, :, None], pv(p, _bf16(v), kvh_true),
                            pv(p, v, kvh_true))
        else:
            o = pv(p, v, kvh_true)
        o = torch.where(l > 0, o / l.clamp_min(1e-300), torch.zeros_like(o))
        ctx = r(o.permute(1, 0, 2).reshape(T, hq * hd))
        a = r(ctx @ L["o"].to(dtype).T)
        prev_kv = (k, v)

        s2 = a + resid
        if resid_twice:
            s2 = torch.where(rows[:, None], s2 + resid, s2)
        h2 = r(norm(s2, L["post_w"]))
        resid = torch.where(rows[:, None], resid, r(s2)) if no_resid_attn else r(s2)
        gu = r(h2 @ L["gate_up"].to(dtype).T)
        g, u = gu[:, : W["inter"]], gu[:, W["inter"]:]
        act = r(g * torch.sigmoid(g) * u)
        pend = r(act @ L["down"].to(dtype).T)
    hidden = r(norm(resid + pend, W["final_w"]))
    logits = r(hidden @ W["lm_head"].to(dtype).T) if want_logits else None
    if want_kv:
        return hidden, logits, own
    return hidden, logits


def oracle(W, script: Script, **kw):
    return forward(W, script.tok, script.positions(), script.count(), **kw)


def emulation(W, script: Script, bf16: bool = True):
    """fp32 with the GPU's bf16 stores (bf16=True) or plain fp32 (the CPU
    engine)."""
    return forward(W, script.tok, script.positions(), script.count(),
                   dtype=torch.float32, rnd=bf16)


# --------------------------------------------------------------------------
# weight mutants
# --------------------------------------------------------------------------
def mutate_weights(W: dict, name: str, layer: int = 1) -> dict:
    M = dict(W)
    Ls = [dict(l) for l in W["layers"]]
    M["layers"] = Ls
    L = Ls[layer]
    hq, hk, hd, inter = W["hq"], W["hk"], W["hd"], W["inter"]
    if name == "norms_exchanged":
        L["in_w"], L["post_w"] = L["post_w"], L["in_w"]
    elif name == "final_norm_ones":
        M["final_w"] = torch.ones_like(W["final_w"])
    elif name == "norm_layer+1":
        o = Ls[(layer + 1) % len(Ls)]
        L["in_w"], L["post_w"] = W["layers"][(layer + 1) % len(Ls)]["in_w"], o["post_w"]
    elif name == "norm_layer-1":
        o = W["layers"][layer - 1]
        L["in_w"], L["post_w"] = o["in_w"], o["post_w"]
    elif name == "kv_exchanged":
        w = L["qkv"].clone()
        a, b = hq * hd, (hq + hk) * hd
        w[a:b], w[b:] = L["qkv"][b:], L["qkv"][a:b]
        L["qkv"] = w
    elif name == "gate_up_exchanged":
        L["gate_up"] = torch.cat([L["gate_up"][inter:], L["gate_up"][:inter]])
    elif name == "rope_rolled":
        M["cos"], M["sin"] = W["cos"].roll(1, 0), W["sin"].roll(1, 0)
    else:
        raise KeyError(name)
    return M


WEIGHT_MUTANTS = ["norms_exchanged", "final_norm_ones", "norm_layer+1", "norm_layer-1",
                  "kv_exchanged", "gate_up_exchanged"]


# --------------------------------------------------------------------------
# recorder
# --------------------------------------------------------------------------
@dataclasses.dataclass
class Record:
    prefix: Tuple[int, ...]     # tokens the row was computed for
    kind: str                   # prefill | catchup | verify | append | decode
    B: int
    bucket: int                 # rows the forward ran (== B unless graphed)
    graphed: bool
    row: torch.Tensor           # clone of the hidden row
    rid: int
    pos: int
    call: int                   # index of the forward it came from
    idx: int                    # row index inside that forward's head input
    sampled: Optional[int] = None   # token sampled from this row, if any
    slot: int = -1                  # flat cache slot the row's K/V went to


class Recorder:
    """Wraps a live engine; one Record per hidden row the model computes."""

    def __init__(self, engine):
        self.e = engine
        self.records: List[Record] = []
        self.padding_rows = 0
        self.preemptions = 0
        self.calls: List[dict] = []       # per forward: head input and kind
        self.prompt_len: Dict[int, int] = {}
        self._kind = "prefill"
        self._nested = False
        e = engine
        self._orig = {}
        for name, kind in (("_prefill_chunk", "prefill"), ("_catchup_forward", "catchup"),
                           ("_spec_verify", "verify"), ("_append_step", "append")):
            self._wrap_kind(name, kind)
        fwd = e.model.forward
        self._orig["model.forward"] = fwd

        def forward_w(fb, *a, **k):
            hidden = fwd(fb, *a, **k)
            if fb.kind != "decode":
                self._take_rows(fb, hidden)
            return hidden

        e.model.forward = forward_w
        for name, graphed in (("_decode_hidden_graphed", True), ("_decode_hidden_eager", False)):
            self._wrap_decode(name, graphed)
        pre = e._preempt
        self._orig["_preempt"] = pre

        def preempt_w(req):
            self.preemptions += 1
            return pre(req)

        e._preempt = preempt_w

    def close(self):
        e = self.e
        del e.model.forward
        for name in ("_prefill_chunk", "_catchup_forward", "_spec_verify", "_append_step",
                     "_decode_hidden_graphed", "_decode_hidden_eager", "_preempt"):
            e.__dict__.pop(name, None)

    def _wrap_kind(self, name, kind):
        orig = getattr(self.e, name)

        def w(*a, **k):
            old, self._kind = self._kind, kind
            try:
                return orig(*a, **k)
            finally:
                self._kind = old

        setattr(self.e, name, w)

    def _owner(self, slot: int, pos: int):
        bs = self.e.kv.block_size
        assert slot % bs == pos % bs, f"slot {slot} does not hold position {pos}"
        blk, bi = slot // bs, pos // bs
        own = [r for r in self.e.running
               if r.seq is not None and len(r.seq.blocks) > bi and r.seq.blocks[bi] == blk]
        assert len(own) == 1, f"row at slot {slot} / position {pos} has {len(own)} owners"
        return own[0]

    def _take_rows(self, fb, hidden):
        ids = fb.input_ids.cpu().tolist()
        pos = fb.positions.cpu().tolist()
        slots = fb.slot_mapping.cpu().tolist()
        assert hidden.shape[0] == len(ids)
        call = len(self.calls)
        rows = hidden.detach().clone()
        kind = self._kind
        label = kind if fb.kind == "prefill" or kind == "append" else kind + "+append"
        run: Dict[int, List[int]] = {}
        first: Dict[int, int] = {}
        for t, (tok, p, s) in enumerate(zip(ids, pos, slots)):
            req = self._owner(s, p)
            toks = req.seq.token_ids
            if req.req_id not in run:
                run[req.req_id] = []
                first[req.req_id] = p
            mine = run[req.req_id]
            assert p == first[req.req_id] + len(mine), "rows of one owner are not consecutive"
            if p < len(toks):
                assert toks[p] == tok, "input id is not the owner's token at that position"
            mine.append(tok)
            prefix = tuple(toks[: first[req.req_id]]) + tuple(mine)
            self.records.append(Record(prefix, label, len(run), len(ids), False,
                                       rows[t], req.req_id, p, call, t, slot=s))
        B = len(run)
        for r in self.records[-len(ids):]:
            r.B = B
        # the rows the engine hands to the head in this kind of step
        if kind == "verify":
            head_rows = list(range(len(ids)))
        elif kind == "append":
            head_rows = (fb.cu_q[1:] - 1).cpu().tolist()
        else:
            head_rows = [len(ids) - 1]
        self.calls.append(dict(kind=kind, hidden=rows, head_rows=head_rows))
        self._after_rows(self.records[-len(ids):])

    def _after_rows(self, recs):
        """Called with the new records once their forward has returned."""

    def _wrap_decode(self, name, graphed):
        orig = getattr(self.e, name)

        def w(B, in_cpu, pos_cpu, slot_cpu, len_cpu, bt_cpu):
            nested, self._nested = self._nested, True
            try:
                hidden = orig(B, in_cpu, pos_cpu, slot_cpu, len_cpu, bt_cpu)
            finally:
                self._nested = nested
            if nested:          # the graphed entry fell back to the eager one
                return hidden
            was_graphed = graphed and self.e.use_hipgraph
            rows = hidden.detach().clone()     # the graph's buffer is static
            bucket = rows.shape[0]
            assert bucket >= B
            self.padding_rows += bucket - B
            call = len(self.calls)
            for i in range(B):
                p, tok, s = int(pos_cpu[i]), int(in_cpu[i]), int(slot_cpu[i])
                req = self._owner(s, p)
                toks = req.seq.token_ids
                assert p + 1 == len(toks) and toks[p] == tok
                self.records.append(Record(tuple(toks), "decode", B, bucket, was_graphed,
                                           rows[i], req.req_id, p, call, i, slot=s))
            self.calls.append(dict(kind="decode", hidden=rows, head_rows=list(range(B))))
            self._after_rows(self.records[-B:])
            return hidden

        setattr(self.e, name, w)

    # -- driving -----------------------------------------------------------
    def add(self, prompt, params) -> int:
        rid = self.e.add_request(list(prompt), params)
        self.prompt_len[rid] = len(prompt)
        return rid

    def _len(self, rid):
        return self.prompt_len[rid] + len(self.e.requests[rid].output_ids)

    def step(self):
        live = [rid for rid in self.prompt_len if rid in self.e.requests]
        before = {rid: self._len(rid) for rid in live}
        n0 = len(self.records)
        self.e.step()
        for rec in self.records[n0:]:
            if rec.rid not in before:
                continue
            if before[rec.rid] <= rec.pos + 1 < self._len(rec.rid):
                rec.sampled = self.history(rec.rid)[rec.pos + 1]
                assert tuple(self.history(rec.rid)[: rec.pos + 1]) == rec.prefix

    def history(self, rid) -> List[int]:
        req = self.e.requests[rid]
        if req.seq is not None:
            return list(req.seq.token_ids)
        return list(req.prompt_ids)

    def run(self, rids, max_steps: int = 4000):
        n = 0
        while not all(self.e.requests[r].finished for r in rids):
            self.step()
            n += 1
            assert n < max_steps, "engine did not finish"

    def pop(self, rid) -> List[int]:
        req = self.e.requests.pop(rid)
        return req.output_ids


# --------------------------------------------------------------------------
# checks shared by the CPU and the GPU test
# --------------------------------------------------------------------------
def script_of(records: Sequence[Record]) -> Tuple[Script, List[int], List[int]]:
    """A trie of the recorded prefixes as one Script. Returns (script, entry
    index per record, root sequence number per entry)."""
    sc = Script()
    node: Dict[Tuple[int, ...], int] = {}
    chains: Dict[Tuple[int, ...], List[int]] = {(): []}
    root_of: List[int] = []
    roots: Dict[int, int] = {}
    for pre in sorted({r.prefix for r in records}, key=len):
        # longest known ancestor
        k = len(pre)
        while pre[:k] not in chains:
            k -= 1
        chain = chains[pre[:k]]
        for d in range(k, len(pre)):
            chain = sc.add([pre[d]], parent=chain, fork=d)
            chains[pre[: d + 1]] = chain
            root = chain[0]
            root_of.append(roots.setdefault(root, len(roots)))
    where = [chains[r.prefix][-1] for r in records]
    return sc, where, root_of


def check_rows(W, records: Sequence[Record], bf16: bool, W_true: Optional[dict] = None):
    """Every record against the oracle of its own prefix. Returns a dict with
    N (per root sequence), the per-record err / T and the oracle rows."""
    sc, where, root_of = script_of(records)
    hid, logits = oracle(W, sc)
    ehid, elog = emulation(W, sc, bf16)
    nroot = max(root_of) + 1
    roots = torch.tensor(root_of)
    N, NL = [], []
    for g in range(nroot):
        sel = roots == g
        N.append(row_rel_err(ehid[sel], hid[sel]))
        NL.append(row_rel_err(elog[sel], logits[sel]))
    out = []
    for rec, i in zip(records, where):
        g = root_of[i]
        e = row_rel_err(rec.row.float()[None], hid[i][None])
        out.append(e / (TOL_FACTOR * N[g]))
    return dict(N=N, NL=NL, ratio=out, hidden=hid, logits=logits, where=where,
                root_of=root_of, script=sc)


def expected_token(engine, rec: Record, recorder: Recorder, params) -> int:
    """The token rule: the head on the rows the engine's own step handed it,
    the engine's arithmetic for bias and penalties, bf16 on the GPU, largest
    value, lowest index on ties."""
    call = recorder.calls[rec.call]
    hidden = call["hidden"]
    if call["kind"] in ("decode", "verify"):      # the head sees every row
        lg = engine.model.compute_logits(hidden)[rec.idx]
    elif call["kind"] == "append":
        hr = call["head_rows"]
        lg = engine.model.compute_logits(hidden[torch.tensor(hr, device=hidden.device)])[
            hr.index(rec.idx)]
    else:
        lg = engine.model.compute_logits(hidden[rec.idx: rec.idx + 1])[0]
    lf = lg.float()
    V = lf.shape[0]
    if params.needs_logit_transform():
        if params.logit_bias:
            for t, b in params.logit_bias.items():
                if 0 <= int(t) < V:
                    lf[int(t)] += float(b)
        outs = rec.prefix[recorder.prompt_len[rec.rid]:]
        if (params.presence_penalty or params.frequency_penalty) and outs:
            cnt = torch.bincount(torch.tensor(outs, device=lf.device), minlength=V)[:V].to(lf.dtype)
            lf -= params.frequency_penalty * cnt + params.presence_penalty * (cnt > 0).to(lf.dtype)
    if lf.is_cuda:
        lf = lf.to(torch.bfloat16).float()
    return int((lf == lf.max()).nonzero()[0])


def check_tokens(engine, recorder: Recorder, params_of: Dict[int, object]) -> int:
    """Asserts the token rule on every sampled row; returns how many."""
    n = 0
    with torch.inference_mode():
        for rec in recorder.records:
            if rec.sampled is None:
                continue
            want = expected_token(engine, rec, recorder, params_of[rec.rid])
            assert want == rec.sampled, (
                f"{rec.kind} row of request {rec.rid} at position {rec.pos}: sampled "
                f"{rec.sampled}, its own hidden state gives {want}")
            n += 1
    return n


# --------------------------------------------------------------------------
# scenarios
# --------------------------------------------------------------------------
SALT = 0   # added to every prompt seed: a run on changed weights must not hit cached prefixes


def rand_ids(seed: int, n: int, vocab: int) -> List[int]:
    g = torch.Generator().manual_seed(seed + SALT)
    return torch.randint(3, vocab, (n,), generator=g).tolist()


def _params(n, **kw):
    from opsagent_amd.engine.engine import SamplingParams

    return SamplingParams(max_new_tokens=n, stop_on_eos=False, **kw)


def sc_solo(rec: Recorder, V: int) -> dict:
    p = _params(40)
    rid = rec.add(rand_ids(11, 70, V), p)
    rec.run([rid])
    return {rid: p}


def sc_batch(rec: Recorder, V: int) -> dict:
    ps = {}
    for i, (n, m) in enumerate(zip((1, 31, 32, 33, 95), (3, 6, 12, 20, 28))):
        p = _params(m)
        ps[rec.add(rand_ids(20 + i, n, V), p)] = p
    rec.run(list(ps))
    return ps


def sc_chunked(rec: Recorder, V: int) -> dict:
    old = rec.e.max_prefill_chunk
    rec.e.max_prefill_chunk = 48
    try:
        p = _params(6)
        rid = rec.add(rand_ids(31, 150, V), p)
        rec.run([rid])
    finally:
        rec.e.max_prefill_chunk = old
    return {rid: p}


def sc_prefix(rec: Recorder, V: int) -> dict:
    shared = rand_ids(41, 100, V)
    p = _params(6)
    a = rec.add(shared + rand_ids(42, 30, V), p)
    rec.run([a])
    before = rec.e.kv.stats["reused_blocks"]
    b = rec.add(shared + rand_ids(43, 30, V), p)
    rec.run([b])
    assert rec.e.kv.stats["reused_blocks"] - before == 3, "96 tokens must be reused"
    rows_b = [r for r in rec.records if r.rid == b and r.kind == "prefill"]
    assert min(r.pos for r in rows_b) == 96
    # a prompt of exactly 96 tokens whose blocks are all cached
    whole = rand_ids(44, 96, V)
    c = rec.add(whole, p)
    rec.run([c])
    before = rec.e.kv.stats["reused_blocks"]
    d = rec.add(whole, p)
    rec.run([d])
    assert rec.e.kv.stats["reused_blocks"] - before == 2   # one token is always recomputed
    return {a: p, b: p, c: p, d: p}


def sc_preempt(rec: Recorder, V: int) -> dict:
    kv = rec.e.kv
    spare = kv.num_free() - 10          # three requests need 12 blocks at 97 tokens
    assert spare >= 0
    held = [kv.alloc_block() for _ in range(spare)]
    try:
        ps = {}
        for i in range(3):
            p = _params(40)
            ps[rec.add(rand_ids(50 + i, 60, V), p)] = p
        n0 = rec.preemptions
        rec.run(list(ps))
        assert rec.preemptions > n0, "the cache was meant to be too small"
    finally:
        for b in held:
            kv.release(b)
    return ps


def sc_verify(rec: Recorder, V: int, exact: bool) -> dict:
    """Proposals from a plain run's own continuation with one wrong token
    planted at index 3, injected at three points; then a repeated-motif
    prompt that the engine's own n-gram lookup serves."""
    e = rec.e
    prompt = rand_ids(61, 50, V)
    p = _params(30)
    plain = rec.add(prompt, p)
    rec.run([plain])
    cont = list(e.requests[plain].output_ids)
    old = (e.spec_decode, e.spec_min_ema, e.spec_ema)
    e.spec_decode, e.spec_min_ema = True, 0.0
    out = {plain: p}
    try:
        rid = rec.add(prompt, p)
        out[rid] = p
        req = e.requests[rid]
        done = set()
        n = 0
        while not req.finished:
            k = len(req.output_ids)
            if (k in (1, 10, 19) and k not in done and not req.spec_tokens
                    and req.seq is not None and req.seq.num_cached == len(req.seq.token_ids) - 1):
                done.add(k)
                props = cont[k: k + 6]
                props[3] = (props[3] + 1) % V
                if props[3] < 3:
                    props[3] += 3
                passes, acc = e.spec_stats["verify_passes"], e.spec_stats["accepted"]
                req.spec_tokens = list(props)
                rec.step()
                assert e.spec_stats["verify_passes"] == passes + 1
                if exact:
                    assert e.spec_stats["accepted"] - acc == 3, "accepted up to the wrong token"
            else:
                rec.step()
            n += 1
            assert n < 500
        assert done == {1, 10, 19}
        if exact:
            assert list(req.output_ids) == cont
        motif = rand_ids(62, 5, V)
        pm = _params(30)
        m = rec.add(motif * 10, pm)
        out[m] = pm
        rec.run([m])
    finally:
        e.spec_decode, e.spec_min_ema, e.spec_ema = old
    return out


def sc_catchup(rec: Recorder, V: int) -> dict:
    """Tokens appended behind the engine's back, as grammar fast-forward
    does: 2, 5 and 17 of them on the first of three running requests."""
    e = rec.e
    ps = {}
    for i, n in enumerate((40, 45, 50)):
        p = _params(60)
        ps[rec.add(rand_ids(70 + i, n, V), p)] = p
    rids = list(ps)
    req = e.requests[rids[0]]
    for j, L in enumerate((2, 5, 17)):
        target = len(req.output_ids) + 3
        n = 0
        while len(req.output_ids) < target or (
                len(req.seq.token_ids) - req.seq.num_cached != 1):
            rec.step()
            n += 1
            assert n < 200 and not req.finished
        extra = rand_ids(80 + j, L, V)
        req.seq.token_ids.extend(extra)
        req.output_ids.extend(extra)
    rec.run(rids)
    return ps


SCENARIOS = {
    "solo": sc_solo, "batch": sc_batch, "chunked": sc_chunked, "prefix": sc_prefix,
    "preempt": sc_preempt, "verify": sc_verify, "catchup": sc_catchup,
}


def run_scenario(name: str, engine, exact: bool = False, recorder=Recorder):
    """Runs one scenario on a fresh Recorder. Returns (recorder, params)."""
    rec = recorder(engine)
    try:
        V = engine.spec.vocab_size
        ps = sc_verify(rec, V, exact) if name == "verify" else SCENARIOS[name](rec, V)
    finally:
        rec.close()
    return rec, ps


# --------------------------------------------------------------------------
# scripted sequences of the scenarios' shapes, and the mutants on them
# --------------------------------------------------------------------------
@dataclasses.dataclass
class Scripted:
    name: str
    script: Script
    chains: List[List[int]]                 # one per sequence
    prompt: List[int]                       # prompt length per sequence
    groups: List[Tuple[int, int, int]]      # (sequence, start, end): multi-token
    #                                         forwards over a cached past
    branch: Optional[List[int]] = None      # chain of a rejected proposal run
    fork: int = 0

    def decode_rows(self) -> torch.Tensor:
        """Entries computed by a decode step: behind the prompt, outside
        every multi-token group."""
        d = torch.zeros(len(self.script), dtype=torch.bool)
        for c, n in zip(self.chains, self.prompt):
            d[c[n:]] = True
        for s, a, b in self.groups:
            d[self.chains[s][a:b]] = False
        return d


def scripted(name: str, V: int) -> Scripted:
    sc = Script()
    if name == "solo":
        return Scripted(name, sc, [sc.add(rand_ids(11, 110, V))], [70], [])
    if name == "batch":
        chains, prompts = [], []
        for i, (n, m) in enumerate(zip((1, 31, 32, 33, 95), (3, 6, 12, 20, 28))):
            chains.append(sc.add(rand_ids(20 + i, n + m, V)))
            prompts.append(n)
        return Scripted(name, sc, chains, prompts, [])
    if name == "chunked":
        c = sc.add(rand_ids(31, 156, V))
        return Scripted(name, sc, [c], [150], [(0, 48, 96), (0, 96, 144), (0, 144, 150)])
    if name == "prefix":
        a = sc.add(rand_ids(41, 100, V) + rand_ids(42, 36, V))
        b = sc.add(rand_ids(43, 36, V), parent=a, fork=100)
        # the second request prefills 96.. over the reused blocks; 96..99 are
        # entries it shares with the first, so the group starts at 100
        return Scripted(name, sc, [a, b], [130, 130], [(1, 100, 130)])
    if name == "verify":
        main = sc.add(rand_ids(61, 80, V))
        br = sc.add(rand_ids(63, 3, V), parent=main, fork=54)
        # one verify forward: positions 50..56, three accepted, three rejected
        return Scripted(name, sc, [main], [50], [(0, 50, 54)], branch=br, fork=54)
    if name == "catchup":
        c = sc.add(rand_ids(70, 40 + 3 + 2 + 3 + 5 + 3 + 17 + 8, V))
        return Scripted(name, sc, [c], [40], [(0, 43, 45), (0, 48, 53), (0, 56, 73)])
    raise KeyError(name)


SCRIPTED = ["solo", "batch", "chunked", "prefix", "verify", "catchup"]
ROW_MUTANTS = [
    "pos+1", "pos-1", "newest_key_dropped", "chunk_ignores_past", "chunk_pos_restart",
    "past_blocks_rolled", "one_block_too_many", "next_row_block_table",
    "padding_writes_row1", "stale_rejected_kv", "cu_q_off", "no_causal_appended",
    "kv_prev_layer", "no_resid_attn", "resid_twice", "head_shift", "k_unroped",
]
ALL_MUTANTS = ROW_MUTANTS + WEIGHT_MUTANTS


def mutant_kwargs(S: Scripted, name: str, W: dict) -> Optional[dict]:
    """forward() arguments that give the answer of one wrong engine on the
    scripted sequences; None where the scenario has no such step."""
    sc = S.script
    pos, count = sc.positions(), sc.count()
    zeros = torch.zeros(len(sc), dtype=torch.float64)
    dec = S.decode_rows()
    kw = dict(W=W, pos=pos, count=count, zeros=zeros)
    if name in WEIGHT_MUTANTS:
        kw["W"] = mutate_weights(W, name)
        return kw
    if name in ("pos+1", "pos-1"):
        pos[dec] += 1 if name == "pos+1" else -1
        return kw
    if name == "newest_key_dropped":
        idx = dec.nonzero().flatten()
        count[idx, idx] = 0
        return kw
    if name in ("kv_prev_layer", "no_resid_attn", "resid_twice", "head_shift", "k_unroped"):
        kw.update({name: True, "rows": dec})
        return kw
    groups = S.groups
    if name in ("chunk_ignores_past", "chunk_pos_restart", "past_blocks_rolled",
                "cu_q_off", "no_causal_appended"):
        if not groups:
            return None
        for s, a, b in groups:
            c = S.chains[s]
            rows = c[a:b] + (S.branch if S.branch is not None else [])
            end = a + len(rows)
            full = c[:a] + rows            # entry per position, as this forward sees it
            for l, i in enumerate(rows):
                if name == "chunk_ignores_past":
                    count[i, c[:a]] = 0
                elif name == "chunk_pos_restart":
                    pos[i] -= a
                elif name == "cu_q_off":
                    count[i, i] = 0
                elif name == "no_causal_appended":
                    count[i] = 0
                    count[i, full] = 1
                else:
                    nblk = -(-end // BLOCK)
                    count[i] = 0
                    for j in range(a + l + 1):
                        pj = ((j // BLOCK + 1) % nblk) * BLOCK + j % BLOCK
                        if pj < end:
                            count[i, full[pj]] += 1
                        else:
                            zeros[i] += 1
        return kw
    if name == "one_block_too_many":
        if S.name != "prefix":
            return None
        a, b = S.chains
        for i in b[128:]:
            count[i, b[96:128]] = 0
            count[i, a[96:128]] = 1
        return kw
    if name in ("next_row_block_table", "padding_writes_row1"):
        if len(S.chains) < 2 or S.name == "prefix":
            return None
        if name == "padding_writes_row1":
            c0, c1 = S.chains[0], S.chains[1]
            n0, n1 = S.prompt[0], S.prompt[1]
            for i in c0[n0:]:
                count[i, c0[n0]] = 0
                count[i, c1[n1]] = 1
            return kw
        nseq = len(S.chains)
        for b in range(nseq):
            c, n = S.chains[b], S.prompt[b]
            o, no = S.chains[(b + 1) % nseq], S.prompt[(b + 1) % nseq]
            i = c[n]
            have = min(n + 1, no + 1)
            count[i] = 0
            count[i, o[:have]] = 1
            zeros[i] = n + 1 - have
        return kw
    if name == "stale_rejected_kv":
        if S.branch is None:
            return None
        main = S.chains[0]
        for pb in range(S.fork, len(S.branch)):
            for i in main[pb:]:
                count[i, main[pb]] = 0
                count[i, S.branch[pb]] = 1
        return kw
    raise KeyError(name)


def mutant_margin(S: Scripted, name: str, W: dict, ref: torch.Tensor, N: float):
    """err(mutant, oracle) / T on the scripted scenario, None where the
    mutant does not apply."""
    kw = mutant_kwargs(S, name, W)
    if kw is None:
        return None
    Wm = kw.pop("W")
    got, _ = forward(Wm, S.script.tok, want_logits=False, **kw)
    return row_rel_err(got, ref) / (TOL_FACTOR * N)
