"""rmsnorm, fused_add_rmsnorm, rope, rope_kv, silu_mul and kv_write on a real
MI355X (`pytest -m gpu`) against fp64 oracles on the exact operands, judged
element by element with the rounding test of tests/pointwise_cases.py:

    |got - r| <= ulp_bf16(r) / 2 + E

Cases, oracles and E come from tests/pointwise_cases.py and are proven able to
fail by tests/test_pointwise_oracle.py. The raw C entries are called so every
output (and every buffer a kernel updates in place) sits inside a larger
buffer filled with a bit pattern: zero failing elements, every bit outside
unchanged, inputs unchanged. Each comparison prints
`POINTWISE <family> | <case> elements failures worst` (visible with -s), where
worst is the largest (|got - r| - ulp/2) / E; the last test prints the
per-family table.
"""

import collections

import numpy as np
import pytest
import torch

import pointwise_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda"
_report = collections.defaultdict(lambda: [0, 0, float("-inf")])


def _lib():
    from opsagent_amd.ops import hip_lib

    return hip_lib, hip_lib.get_lib()


def dev_bits(bits) -> torch.Tensor:
    """uint16 bf16 bits -> bf16 tensor on the GPU, same shape."""
    a = np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)
    return torch.from_numpy(a.copy()).to(DEV).view(torch.bfloat16)


def dev_vals(x) -> torch.Tensor:
    return dev_bits(pc.to_bits(x).reshape(np.shape(x)))


def host_bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


class Guard:
    """`shape` bf16 elements inside a longer buffer filled with PATTERN bits."""

    def __init__(self, shape, init=None, pad=None):
        self.n = int(np.prod(shape))
        self.pad = pad or 64                          # elements; keeps the view 16-byte aligned
        assert self.pad % 8 == 0
        full = np.full(self.n + 2 * self.pad, pc.PATTERN, dtype=np.uint16)
        if init is not None:
            full[self.pad:self.pad + self.n] = np.asarray(init, dtype=np.uint16).reshape(-1)
        self.buf = dev_bits(full)
        self.t = self.buf[self.pad:self.pad + self.n].view(*shape)

    def bits(self) -> np.ndarray:
        return host_bits(self.t)

    def assert_outside_untouched(self, msg):
        b = host_bits(self.buf)
        assert (b[:self.pad] == pc.PATTERN).all(), f"{msg}: wrote before the buffer"
        assert (b[self.pad + self.n:] == pc.PATTERN).all(), f"{msg}: wrote past the buffer"


def _account(family, case, v):
    r = _report[family]
    r[0], r[1], r[2] = r[0] + v.n, r[1] + v.fails, max(r[2], v.worst)
    print(f"\nPOINTWISE {family} | {case.name} elements={v.n} failures={v.fails} worst={v.worst:.3f}  [{v}]")
    assert v.fails == 0, f"{case.name}: {v}"


# --------------------------------------------------------------------------
# rmsnorm / fused add
# --------------------------------------------------------------------------
def launch_norm(case: pc.NormCase, w=None):
    """Through oa_rmsnorm / oa_fused_add_rmsnorm; returns (rc, got, guards).
    The buffers hold rows + 2 rows and the launch is told `rows`."""
    hip_lib, lib = _lib()
    rows, dim = case.rows, case.dim
    x = dev_vals(case.x)
    wt = dev_vals(case.w if w is None else w)
    out = Guard((rows, dim), pad=max(dim, 64))
    stream = hip_lib.current_stream_ptr()
    guards = {"out": out}
    if case.fused:
        res = Guard((rows, dim), init=pc.to_bits(case.res), pad=max(dim, 64))
        guards["res"] = res
        rc = lib.oa_fused_add_rmsnorm(stream, x.data_ptr(), res.t.data_ptr(), wt.data_ptr(),
                                      out.t.data_ptr(), rows, dim, case.eps)
    else:
        rc = lib.oa_rmsnorm(stream, x.data_ptr(), wt.data_ptr(), out.t.data_ptr(), rows, dim, case.eps)
    torch.cuda.synchronize()
    assert np.array_equal(host_bits(x), pc.to_bits(case.x)), "x changed"
    return rc, {k: g.bits() for k, g in guards.items()}, guards


def _norm_id(k):
    return f"{'fused-' if k[3] else ''}d{k[0]}-r{k[1]}-eps{k[2]:g}"


@pytest.mark.parametrize("key", pc.norm_keys(), ids=_norm_id)
def test_rmsnorm(key):
    case = pc.norm_case(*key)
    rc, got, guards = launch_norm(case)
    assert rc == 0, f"{case.name}: rc={rc}"
    for g in guards.values():
        g.assert_outside_untouched(case.name)
    _account("fused_add_rmsnorm" if case.fused else "rmsnorm", case, case.verdict(got))


def test_rmsnorm_public_wrappers():
    from opsagent_amd import ops

    case = pc.norm_case(4096, 6, 1e-5, False)
    got = ops.rms_norm(dev_vals(case.x), dev_vals(case.w), case.eps)
    assert case.verdict({"out": host_bits(got)}).fails == 0
    case = pc.norm_case(4096, 6, 1e-5, True)
    res = dev_vals(case.res)
    ret = ops.fused_add_rms_norm(dev_vals(case.x), res, dev_vals(case.w), case.eps)
    out, new_res = ret
    assert new_res.data_ptr() == res.data_ptr(), "the returned residual is the input's buffer"
    assert case.verdict({"out": host_bits(out), "res": host_bits(new_res)}).fails == 0


@pytest.mark.parametrize("dim", [12, 8200])
def test_rmsnorm_launcher_rejects(dim):
    hip_lib, lib = _lib()
    x = torch.zeros(2, 8208, dtype=torch.bfloat16, device=DEV)
    out = Guard((2, 8208))
    stream = hip_lib.current_stream_ptr()
    assert lib.oa_rmsnorm(stream, x.data_ptr(), x.data_ptr(), out.t.data_ptr(), 2, dim, 1e-5) == -100
    res = Guard((2, 8208))
    assert lib.oa_fused_add_rmsnorm(stream, x.data_ptr(), res.t.data_ptr(), x.data_ptr(),
                                    out.t.data_ptr(), 2, dim, 1e-5) == -100
    torch.cuda.synchronize()
    assert (out.bits() == pc.PATTERN).all() and (res.bits() == pc.PATTERN).all()


# --------------------------------------------------------------------------
# rope / rope_kv
# --------------------------------------------------------------------------
def launch_rope(case: pc.RopeCase, cos=None, sin=None):
    hip_lib, lib = _lib()
    T, Hq, Hk, D = case.T, case.Hq, case.Hk, case.D
    cos_t = torch.from_numpy(case.cos if cos is None else cos).to(DEV).contiguous()
    sin_t = torch.from_numpy(case.sin if sin is None else sin).to(DEV).contiguous()
    pos = torch.from_numpy(case.pos).to(DEV)
    stream = hip_lib.current_stream_ptr()
    if case.kind == "rope":
        q = Guard((T, Hq, D), init=pc.to_bits(case.q))
        k = Guard((T, Hk, D), init=pc.to_bits(case.k))
        rc = lib.oa_rope(stream, q.t.data_ptr(), k.t.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(),
                         pos.data_ptr(), T, Hq, Hk, D)
        torch.cuda.synchronize()
        guards = [q, k]
        got = {"q": q.bits(), "k": k.bits()}
    else:
        # q, k, v: head slices of one buffer whose token stride has 8 columns of padding
        cols = (Hq + 2 * Hk) * D
        stride = cols + 8
        img = np.full((T, stride), pc.PATTERN, dtype=np.uint16)
        img[:, :Hq * D] = pc.to_bits(case.q).reshape(T, -1)
        img[:, Hq * D:(Hq + Hk) * D] = pc.to_bits(case.k).reshape(T, -1)
        img[:, (Hq + Hk) * D:cols] = case.v.reshape(T, -1)
        qkv = Guard((T, stride), init=img)
        kc = Guard((case.S, Hk, D), init=case.kc0)
        vc = Guard((case.S, Hk, D), init=case.vc0)
        slots = torch.from_numpy(case.slots).to(DEV)
        base = qkv.t.data_ptr()
        rc = lib.oa_rope_kv(stream, base, base + 2 * Hq * D, base + 2 * (Hq + Hk) * D,
                            kc.t.data_ptr(), vc.t.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(),
                            pos.data_ptr(), slots.data_ptr(), T, Hq, Hk, D, stride, stride, stride)
        torch.cuda.synchronize()
        guards = [qkv, kc, vc]
        after = qkv.bits()
        assert (after[:, cols:] == pc.PATTERN).all(), f"{case.name}: padding columns changed"
        assert np.array_equal(after[:, (Hq + Hk) * D:cols], case.v.reshape(T, -1)), f"{case.name}: v changed"
        got = {"q": after[:, :Hq * D].reshape(T, Hq, D), "k": after[:, Hq * D:(Hq + Hk) * D].reshape(T, Hk, D),
               "kc": kc.bits(), "vc": vc.bits()}
    for g in guards:
        g.assert_outside_untouched(case.name)
    return rc, got


_ROPE_KEYS = pc.rope_keys("rope") + pc.rope_keys("rope_kv")


@pytest.mark.parametrize("key", _ROPE_KEYS, ids=lambda k: f"{k[0]}-t{k[1]}-hq{k[2]}-hk{k[3]}-d{k[4]}")
def test_rope(key):
    case = pc.rope_case(*key)
    rc, got = launch_rope(case)
    assert rc == 0, f"{case.name}: rc={rc}"
    _account(case.kind, case, case.verdict(got))


def test_rope_kv_launcher_rejects():
    hip_lib, lib = _lib()
    buf = Guard((4, 1024))
    cache = Guard((8, 256))
    f = torch.zeros(97 * 128, dtype=torch.float32, device=DEV)
    i = torch.zeros(4, dtype=torch.int32, device=DEV)
    s, p = hip_lib.current_stream_ptr(), buf.t.data_ptr()
    args = (s, p, p + 512, p + 1024, cache.t.data_ptr(), cache.t.data_ptr(), f.data_ptr(), f.data_ptr(),
            i.data_ptr(), i.data_ptr(), 1, 1, 1)
    assert lib.oa_rope_kv(*args, 24, 1024, 1024, 1024) == -100
    assert lib.oa_rope_kv(*args, 32, 1028, 1024, 1024) == -101
    assert lib.oa_rope_kv(*args, 32, 1024, 1024, 1020) == -101
    assert lib.oa_rope(s, p, p + 512, f.data_ptr(), f.data_ptr(), i.data_ptr(), 1, 1, 1, 24) == -100
    torch.cuda.synchronize()
    assert (buf.bits() == pc.PATTERN).all() and (cache.bits() == pc.PATTERN).all()


def _qkv_views(case, v_bits):
    """q, k, v as head slices of one fused buffer, as the engine passes them."""
    T, Hq, Hk, D = case.T, case.Hq, case.Hk, case.D
    img = np.concatenate([pc.to_bits(case.q).reshape(T, -1), pc.to_bits(case.k).reshape(T, -1),
                          np.asarray(v_bits).reshape(T, -1)], axis=1)
    raw = dev_bits(img)
    return (raw, raw[:, :Hq * D].view(T, Hq, D), raw[:, Hq * D:(Hq + Hk) * D].view(T, Hk, D),
            raw[:, (Hq + Hk) * D:].view(T, Hk, D))


@pytest.mark.parametrize("key", [("rope_kv", 37, 6, 2, 128), ("rope_kv", 1, 5, 3, 128)],
                         ids=lambda k: f"t{k[1]}-hq{k[2]}-hk{k[3]}")
def test_rope_kv_fp8_rope(key):
    """The rope of rope_kv_fp8 on the same tables: q and the in-place k by the
    criterion (its codes and scales are proven against those rows elsewhere).
    v is finite here: it is quantised."""
    from opsagent_amd import ops

    case = pc.rope_case(*key)
    T, Hk, D = case.T, case.Hk, case.D
    v = pc.to_bits(pc.bf16_round(np.random.default_rng(T).standard_normal((T, Hk, D)).astype(np.float32)))
    raw, q, k, vv = _qkv_views(case, v)
    bs = 8
    nb = -(-case.S // bs)
    codes = [torch.zeros(nb, bs, Hk, D, dtype=torch.uint8, device=DEV) for _ in range(2)]
    scales = [torch.zeros(nb, bs, Hk, dtype=torch.float32, device=DEV) for _ in range(2)]
    ops.rope_kv_fused_fp8(q, k, vv, codes[0], codes[1], scales[0], scales[1],
                          torch.from_numpy(case.cos).to(DEV), torch.from_numpy(case.sin).to(DEV),
                          torch.from_numpy(case.pos).to(DEV), torch.from_numpy(case.slots).to(DEV))
    torch.cuda.synchronize()
    assert np.array_equal(host_bits(vv), v), "v changed"
    v_ = pc.Verdict()
    v_.add("q", case.rq.size, *pc.judge(host_bits(q), case.rq, case.Eq))
    v_.add("k", case.rk.size, *pc.judge(host_bits(k), case.rk, case.Ek))
    _account("rope_kv_fp8", case, v_)


_DECODE_RUNS = [(key, ns, fused) for key in pc.decode_rope_keys() for ns in pc.DECODE_NSPLITS
                for fused in (False, True)]


@pytest.mark.parametrize("key,nsplit,fused", _DECODE_RUNS,
                         ids=[f"g{k[0]}-n{'_'.join(map(str, k[1]))}-s{ns}-{'fused' if f else 'two'}"
                              for k, ns, f in _DECODE_RUNS])
def test_decode_rope(key, nsplit, fused):
    """The rope-fused decode (ops.attention_decode_rope, both entries): the k
    row it writes at the new slot by the criterion, the v row bit for bit,
    every other cache bit unchanged."""
    from opsagent_amd import ops

    case = pc.decode_rope_case(*key)
    B, Hk, D, bs = case.T, case.Hk, case.D, pc.DECODE_BS
    raw, q, k, v = _qkv_views(case, case.v)
    before = host_bits(raw)
    kc = Guard((case.S // bs, bs, Hk, D), init=case.kc0)
    vc = Guard((case.S // bs, bs, Hk, D), init=case.vc0)
    out = ops.attention_decode_rope(
        q, k, v, kc.t, vc.t, torch.from_numpy(case.bt).to(DEV), torch.from_numpy(case.lens).to(DEV),
        torch.from_numpy(case.cos).to(DEV), torch.from_numpy(case.sin).to(DEV),
        torch.from_numpy(case.slots).to(DEV), nsplit=nsplit, fused_combine=fused)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    kc.assert_outside_untouched(case.name)
    vc.assert_outside_untouched(case.name)
    assert np.array_equal(host_bits(raw), before), "the raw q, k, v rows changed"
    got = {"kc": kc.bits().reshape(case.S, Hk, D), "vc": vc.bits().reshape(case.S, Hk, D)}
    _account("decode_rope", case, case.verdict(got))


@pytest.mark.parametrize("fused", [False, True], ids=["two", "fused"])
@pytest.mark.parametrize("name", [c[0] for c in pc.ATTENTION_CASES])
def test_decode_attention_on_synthetic_tables(name, fused):
    """The output of the rope-fused decode against the fp64 oracle of
    tests/attention_oracle.py, q roped in fp64 and not rounded, T = 4 N."""
    import attention_oracle as ao
    from opsagent_amd import ops

    c, _ = pc.attention_case(name)
    raw = torch.cat([c.q.flatten(1), c.k_new.flatten(1), c.v_new.flatten(1)], dim=-1).to(DEV)
    D = ao.D_HEAD
    q = raw[:, :c.Hq * D].view(c.B, c.Hq, D)
    k = raw[:, c.Hq * D:(c.Hq + c.Hk) * D].view(c.B, c.Hk, D)
    v = raw[:, (c.Hq + c.Hk) * D:].view(c.B, c.Hk, D)
    out = ops.attention_decode_rope(q, k, v, c.kc.to(DEV), c.vc.to(DEV), c.bt.to(DEV), c.lens.to(DEV),
                                    c.cos.to(DEV), c.sin.to(DEV), c.slots.to(DEV), scale=c.scale,
                                    nsplit=c.nsplit, fused_combine=fused)
    torch.cuda.synchronize()
    err = ao.row_rel_err(out.cpu(), c.ref)
    print(f"\nPOINTWISE decode attention | {name} err={err:.5f} T={c.tol:.5f} ratio={err / c.tol:.3f}")
    assert err <= c.tol, f"{name}: row_rel_err {err:.5f} > T {c.tol:.5f}"


# --------------------------------------------------------------------------
# silu_mul / kv_write
# --------------------------------------------------------------------------
@pytest.mark.parametrize("n", pc.silu_keys())
def test_silu_mul(n):
    hip_lib, lib = _lib()
    case = pc.silu_case(n)
    g, u = dev_vals(case.g), dev_vals(case.u)
    out = Guard((n,))
    rc = lib.oa_silu_mul(hip_lib.current_stream_ptr(), g.data_ptr(), u.data_ptr(), out.t.data_ptr(), n)
    torch.cuda.synchronize()
    assert rc == 0
    out.assert_outside_untouched(case.name)
    assert np.array_equal(host_bits(g), pc.to_bits(case.g)) and np.array_equal(host_bits(u), pc.to_bits(case.u))
    _account("silu_mul", case, case.verdict({"out": out.bits()}))


def test_silu_mul_wrapper_and_rejects():
    from opsagent_amd import ops

    hip_lib, lib = _lib()
    case = pc.silu_case(2056)
    got = ops.silu_mul(dev_vals(case.g), dev_vals(case.u))
    assert case.verdict({"out": host_bits(got)}).fails == 0
    out = Guard((16,))
    z = torch.zeros(16, dtype=torch.bfloat16, device=DEV)
    assert lib.oa_silu_mul(hip_lib.current_stream_ptr(), z.data_ptr(), z.data_ptr(), out.t.data_ptr(), 12) == -100
    torch.cuda.synchronize()
    assert (out.bits() == pc.PATTERN).all()


@pytest.mark.parametrize("key", pc.KV_KEYS, ids=lambda k: f"t{k[0]}-hk{k[1]}-d{k[2]}")
def test_kv_write(key):
    hip_lib, lib = _lib()
    case = pc.kv_write_case(*key)
    kc = Guard((case.S, case.Hk, case.D), init=case.kc0)
    vc = Guard((case.S, case.Hk, case.D), init=case.vc0)
    k, v = dev_bits(case.k), dev_bits(case.v)
    slots = torch.from_numpy(case.slots).to(DEV)
    rc = lib.oa_kv_write(hip_lib.current_stream_ptr(), kc.t.data_ptr(), vc.t.data_ptr(), k.data_ptr(),
                         v.data_ptr(), slots.data_ptr(), case.T, case.Hk, case.D)
    torch.cuda.synchronize()
    assert rc == 0
    kc.assert_outside_untouched(case.name)
    vc.assert_outside_untouched(case.name)
    _account("kv_write", case, case.verdict({"kc": kc.bits(), "vc": vc.bits()}))


def test_kv_write_launcher_rejects():
    hip_lib, lib = _lib()
    cache = Guard((8, 16))
    z = torch.zeros(64, dtype=torch.bfloat16, device=DEV)
    i = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert lib.oa_kv_write(hip_lib.current_stream_ptr(), cache.t.data_ptr(), cache.t.data_ptr(), z.data_ptr(),
                           z.data_ptr(), i.data_ptr(), 1, 1, 12) == -100
    torch.cuda.synchronize()
    assert (cache.bits() == pc.PATTERN).all()


# --------------------------------------------------------------------------
# the comparison itself, checked on the GPU
# --------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
def test_comparison_sees_a_rolled_norm_weight(fused):
    """The real kernel fed w rolled by two elements is the CPU proof's mutant
    `w_rolled_2`: it must pass against that mutant's own oracle with zero
    failures and fail the true one on at least as many elements as the CPU
    mutant does."""
    case = pc.norm_case(2056, 6, 1e-5, fused)
    rc, got, _ = launch_norm(case, w=np.roll(case.w, 2))
    assert rc == 0
    own = case.verdict(got, ref=case.mutant_ref(w_roll=2))
    true = case.verdict(got)
    predicted = case.verdict(case.emulation(w_roll=2)).fails
    print(f"\nPOINTWISE self-check w_rolled_2 | {case.name}: own {own}, true failures {true.fails}, "
          f"CPU mutant {predicted}")
    assert own.fails == 0 and predicted >= pc.MIN_FAIL and true.fails >= predicted


def test_comparison_sees_a_rolled_table():
    """rope_kv fed tables rolled by one position is the mutant `position-1`."""
    case = pc.rope_case("rope_kv", 37, 6, 2, 128)
    cos, sin = np.roll(case.cos, 1, axis=0), np.roll(case.sin, 1, axis=0)
    rc, got = launch_rope(case, cos=cos, sin=sin)
    assert rc == 0
    own = case.verdict(got, ref=case.mutant_ref(cos, sin))
    true = case.verdict(got)
    predicted = case.verdict(case.emulation(pos_shift=-1)).fails
    print(f"\nPOINTWISE self-check table rolled | {case.name}: own {own}, true failures {true.fails}, "
          f"CPU mutant {predicted}")
    assert own.fails == 0 and predicted >= pc.MIN_FAIL and true.fails >= predicted


def test_report():
    """Report only (needs the tests above in the same run)."""
    for fam in sorted(_report):
        n, f, w = _report[fam]
        print(f"\nPOINTWISE table | {fam}: elements={n} failures={f} worst={w:.3f}")
        assert f == 0
