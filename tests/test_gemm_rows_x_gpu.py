"""bf16 GEMM inputs for the 65..128-row launches (fo_gemm_set_x_bf16, x_round="bf16").

The oracle is bit-exact: k_gemm_rows on an X whose elements are bf16 values already splits it into hi = X and lo = +0,
and an MFMA whose A operand is all zeros returns its accumulator, so the armed launch on X must EQUAL the unarmed one on
Xr = X.bfloat16().float() in every tensor it writes (torch.equal; no tolerance).  Around that: armed(Xr) == armed(X);
against float64 on Xr the GEMM tests' bound holds (2e-4 x the reference's max); against float64 on the unrounded X the
error is ABOVE that bound (a build that ignores the arm fails there); and the launch counters show that k_gemm_rows ran
and that exactly the armed launch took the bf16 form.

Shapes: the four ragged ones of test_gemm_gpu.test_gemm_rows_ragged_tile_groups (the smallest that reach k_gemm_rows:
ragged last tile group, uneven K splits; both instantiations of the plain and of the SwiGLU form), the fused q|k|v at
Qwen2 geometry at 65 and 128 rows, and the real 128-row Qwen2 down and gate/up.  The float64 references are taken on
at most 512 fixed output columns (all of them where there are fewer); the bit-exact comparisons cover every element.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
EPS = 1e-6
SENT = -768.0   # (a bf16 value too: the bf16 cache holds it exactly)
NREF = 512   # output columns of the float64 references


@pytest.fixture(autouse=True)
def _counters():
    from fo import _lib, ops
    ops.launch_counts_reset()
    ops.rows_xb_launch_count_reset()
    yield
    _lib.load().fo_gemm_set_x_bf16(0)


def _gen(seed, dev):
    return torch.Generator(device=dev).manual_seed(seed)


def _weight(N, K, g, dev):
    return (torch.randn(N, K, generator=g, device=dev) / K ** 0.5).to(torch.bfloat16)


def _cols(N, seed):
    if N <= NREF:
        return torch.arange(N)
    return torch.randperm(N, generator=torch.Generator().manual_seed(seed))[:NREF].sort().values


class Plain:
    """bias + residual (in place) + stats_out: writes Y, yg and the row-statistics buffer."""

    def __init__(self, M, N, K, dev, bias=True):
        from fo.ops import PackedLinear
        g = _gen(M * 7 + N + K, dev)
        self.M, self.N, self.K, self.dev = M, N, K, dev
        w = _weight(N, K, g, dev)
        self.b = torch.randn(N, generator=g, device=dev) if bias else None
        self.r = torch.randn(M, N, generator=g, device=dev)
        self.gamma = torch.rand(N, generator=g, device=dev) + 0.5
        self.x = torch.randn(M, K, generator=g, device=dev)
        self.lin = PackedLinear(w, self.b)
        self.cols = _cols(N, N + K)
        self.wc = w[self.cols.to(dev)].cpu().double()
        del w

    def run(self, x, x_round=None):
        from fo import ops
        st = ops.RowStats(self.M, self.dev)
        st.buf.fill_(SENT)
        out = self.r.clone()
        yg = torch.full_like(out, SENT)
        self.lin(x, out=out, residual=True, stats_out=st.set(self.gamma, yg), x_round=x_round)
        assert 0 < st.groups <= st.max_groups
        return {"y": out, "yg": yg, "stats": st.buf, "groups": torch.tensor(st.groups)}

    def ref(self, x):
        c = self.cols
        y = x.cpu().double() @ self.wc.t() + self.r.cpu().double()[:, c]
        if self.b is not None:
            y = y + self.b.cpu().double()[c]
        return {"y": y, "yg": y * self.gamma.cpu().double()[c]}

    def pick(self, out):
        c = self.cols.to(self.dev)
        return {"y": out["y"][:, c].cpu().double(), "yg": out["yg"][:, c].cpu().double()}


class SwiGLU:
    """SwiGLU with an RMSNorm consumer (row statistics as a producer leaves them): writes Y."""

    def __init__(self, M, N, K, dev):
        from fo import ops
        from fo.ops import PackedLinear
        g = _gen(M * 7 + N + K, dev)
        self.M, self.N, self.K, self.dev = M, N, K, dev
        w, u = _weight(N, K, g, dev), _weight(N, K, g, dev)
        self.x = torch.randn(M, K, generator=g, device=dev)
        self.lin = PackedLinear(w, swiglu_up=u)
        self.st = ops.RowStats(M, dev)
        self.st.groups = 14   # partial sums of squares of a row of about unit elements, in 14 groups
        self.st.buf[:M * 14] = (torch.rand(M * 14, generator=g, device=dev) + 0.5) * (K / 14)
        self.cols = _cols(N, N + K)
        c = self.cols.to(dev)
        self.wc, self.uc = w[c].cpu().double(), u[c].cpu().double()
        del w, u

    def run(self, x, x_round=None):
        out = torch.full((self.M, self.N), SENT, device=self.dev)
        self.lin(x, out=out, norm=(self.st, EPS), x_round=x_round)
        return {"y": out}

    def ref(self, x):
        ss = self.st.buf[:self.M * 14].view(self.M, 14).cpu().double().sum(1, keepdim=True)
        rs = torch.rsqrt(ss / self.K + EPS)
        xd = x.cpu().double()
        return {"y": torch.nn.functional.silu(rs * (xd @ self.wc.t())) * (rs * (xd @ self.uc.t()))}

    def pick(self, out):
        return {"y": out["y"][:, self.cols.to(self.dev)].cpu().double()}


class QKV:
    """The fused q|k|v at Qwen2 geometry (bias, RoPE, paged-KV append in the reduce) into sentinel-filled caches: writes
    q_out and M rows of K and V; everything else of the caches stays the sentinel."""
    H, KVH, hd, K, PS, pages = 28, 4, 128, 3584, 16, 12

    def __init__(self, M, dev, kv_dtype=torch.float32):
        from fo.ops import PackedLinear
        g = _gen(M * 13 + 5, dev)
        self.M, self.dev, self.kv_dtype = M, dev, kv_dtype
        # (a bf16 cache rounds K / V as it stores them: the float64 bounds are taken on q_out there, the equalities on all)
        self.bound_keys = ("q", "k", "v") if kv_dtype == torch.float32 else ("q",)
        self.N = (self.H + 2 * self.KVH) * self.hd
        half = self.hd // 2
        w = _weight(self.N, self.K, g, dev)
        self.b = torch.randn(self.N, generator=g, device=dev) * 0.1
        self.x = torch.randn(M, self.K, generator=g, device=dev)
        cg = torch.Generator().manual_seed(M)
        self.pos = torch.randint(0, 300, (M,), generator=cg, dtype=torch.int32)
        self.slot = torch.randperm(self.pages * self.PS, generator=cg)[:M].to(torch.int32)
        inv = 1.0 / (1e6 ** (torch.arange(0, half, dtype=torch.float64) / half))
        ang = torch.arange(512, dtype=torch.float64)[:, None] * inv[None]
        self.cos, self.sin = torch.cos(ang).float(), torch.sin(ang).float()
        self.lin = PackedLinear(w, self.b, rope_hd=self.hd)
        self.w = w.cpu().double()   # (4608 x 3584: the whole projection, RoPE pairs columns half a head apart)
        del w

    def run(self, x, x_round=None):
        dev = self.dev
        q = torch.full((self.M, self.H * self.hd), SENT, device=dev)
        kc = torch.full((self.pages, self.KVH, self.PS, self.hd), SENT, device=dev, dtype=self.kv_dtype)
        vc = torch.full_like(kc, SENT)
        self.lin.qkv_rope(x, self.M, self.pos.to(dev), self.slot.to(dev), self.cos.to(dev), self.sin.to(dev), q, kc, vc,
                          self.H, self.KVH, self.PS, x_round=x_round)
        return {"q": q, "k": kc, "v": vc}

    def ref(self, x):
        H, KVH, hd, half = self.H, self.KVH, self.hd, self.hd // 2
        y = x.cpu().double() @ self.w.t() + self.b.cpu().double()
        heads = y.view(self.M, H + 2 * KVH, hd)
        c, s = self.cos.double()[self.pos.long()][:, None, :], self.sin.double()[self.pos.long()][:, None, :]
        x1, x2 = heads[..., :half], heads[..., half:]
        rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
        return {"q": rot[:, :H].reshape(self.M, -1), "k": rot[:, H:H + KVH], "v": heads[:, H + KVH:]}

    def pick(self, out):
        sl = self.slot.long().to(self.dev)
        rows = lambda t: t[sl // self.PS, :, sl % self.PS].cpu().double()
        touched = torch.zeros(self.pages * self.PS, dtype=torch.bool)
        touched[self.slot.long()] = True
        for t in (out["k"], out["v"]):   # the untouched slots still hold the sentinel
            flat = t.float().cpu().permute(0, 2, 1, 3).reshape(self.pages * self.PS, -1)
            assert bool((flat[~touched] == SENT).all()) and not bool((flat[touched] == SENT).any())
        return {"q": out["q"].cpu().double(), "k": rows(out["k"]), "v": rows(out["v"])}


def _equal(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert not torch.isnan(a[k].float()).any(), (what, k)
        assert torch.equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


def _worst(case, out, x):
    """The largest error of the picked outputs against float64 on x, as a fraction of that reference's max."""
    got, ref = case.pick(out), case.ref(x)
    return max(float((got[k] - ref[k]).abs().max() / ref[k].abs().max()) for k in getattr(case, "bound_keys", ref))


def _check(case, what, bound=2e-4):
    from fo import ops
    x = case.x
    xr = x.bfloat16().float()
    assert not torch.equal(x, xr)
    ops.launch_counts_reset()
    ops.rows_xb_launch_count_reset()
    base_r = case.run(xr)
    base = case.run(x)
    assert ops.launch_counts()["gemm_rows"] == 2, (what, ops.launch_counts())
    assert ops.rows_xb_launch_count() == 0, what           # without the arm the counter stays 0
    armed = case.run(x, "bf16")
    assert ops.launch_counts()["gemm_rows"] == 3 and ops.launch_counts()["gemm_reduce"] == 3, what
    assert ops.rows_xb_launch_count() == 1, what           # the shape reached the kernel and took the arm
    armed_r = case.run(xr, "bf16")
    torch.cuda.synchronize()
    assert ops.rows_xb_launch_count() == 2, what
    _equal(armed, base_r, f"{what}: armed(X) vs unarmed(bf16(X))")           # 1
    _equal(armed_r, armed, f"{what}: armed(bf16(X)) vs armed(X)")            # 2
    e_r, e_x, e_base = _worst(case, armed, xr), _worst(case, armed, x), _worst(case, base, x)
    print(f"[rows x bf16] {what}: armed vs float64 on bf16(X) {e_r:.2e}, on X {e_x:.2e}; unarmed on X {e_base:.2e} "
          f"(of the reference's max; bound {bound:.0e})")
    assert e_r < bound, (what, e_r)                                          # 3
    assert e_x > bound, (what, e_x)                                          # 4: the rounding is really there
    assert e_base < bound, (what, e_base)
    # the arm is consumed by its launch: the next one, not re-armed, is the fp32 arm again
    _equal(case.run(x), base, f"{what}: the launch after the armed one")
    assert ops.rows_xb_launch_count() == 2, what


@pytest.mark.parametrize("M,N,K", [(97, 2320, 4096), (128, 4624, 2048)])
def test_plain_bias_residual_stats(dev, M, N, K):
    _check(Plain(M, N, K, dev), f"plain {M} x {N} x {K}")


@pytest.mark.parametrize("M,N,K", [(66, 2208, 3584), (113, 3056, 4096)])
def test_swiglu_with_norm_consumer(dev, M, N, K):
    _check(SwiGLU(M, N, K, dev), f"swiglu {M} x {N} x {K}")


@pytest.mark.parametrize("M,kv", [(65, "fp32"), (128, "fp32"), (128, "bf16")])
def test_qkv_rope(dev, M, kv):
    _check(QKV(M, dev, torch.float32 if kv == "fp32" else torch.bfloat16), f"q|k|v {M} rows, {kv} cache")


def test_qwen2_down_128_rows(dev):
    _check(Plain(128, 3584, 18944, dev, bias=False), "Qwen2 down, 128 rows")


def test_qwen2_gate_up_128_rows(dev):
    _check(SwiGLU(128, 18944, 3584, dev), "Qwen2 gate/up, 128 rows")


# ---------------------------------------------------------------- the arm is a permission
def _ignored(case, run_armed, what):
    """The launch has no use for the arm: outputs bit for bit the unarmed ones, the new counter stays 0."""
    from fo import ops
    ops.rows_xb_launch_count_reset()
    base = case.run(case.x)
    armed = run_armed()
    torch.cuda.synchronize()
    _equal(armed, base, what)
    assert ops.rows_xb_launch_count() == 0, what


def test_arm_ignored_at_64_rows(dev):
    from fo import ops
    case = Plain(64, 2320, 4096, dev)
    _ignored(case, lambda: case.run(case.x, "bf16"), "64 rows")
    assert ops.launch_counts()["gemm_rows"] == 0


def test_arm_ignored_under_16_mib(dev):
    from fo import ops
    case = Plain(100, 1024, 4096, dev)   # 8 MiB of packed weight
    _ignored(case, lambda: case.run(case.x, "bf16"), "8 MiB weight at 100 rows")
    assert ops.launch_counts()["gemm_rows"] == 0


def test_arm_ignored_with_rows_off(dev):
    from fo import _lib, ops
    lib = _lib.load()
    case = Plain(97, 2320, 4096, dev)
    prev = lib.fo_gemm_set_rows(0)
    try:
        _ignored(case, lambda: case.run(case.x, "bf16"), "fo_gemm_set_rows(0)")
        assert ops.launch_counts()["gemm_rows"] == 0
    finally:
        lib.fo_gemm_set_rows(prev)


def test_arm_ignored_for_bf16_x(dev):
    from fo import ops
    case = Plain(97, 2320, 4096, dev)
    case.x = case.x.bfloat16()
    _ignored(case, lambda: case.run(case.x, "bf16"), "bf16 X tensor")
    assert ops.launch_counts()["gemm_rows"] == 0


def test_arm_is_consumed_by_a_launch_that_has_no_use_for_it(dev):
    """Armed through the C-ABI, then a 64-row launch (which ignores it): the 97-row launch after it runs unarmed."""
    from fo import _lib, ops
    lib = _lib.load()
    small, case = Plain(64, 2320, 4096, dev), Plain(97, 2320, 4096, dev)
    base = case.run(case.x)
    assert lib.fo_gemm_set_x_bf16(1) == 0
    small.run(small.x)
    got = case.run(case.x)
    torch.cuda.synchronize()
    _equal(got, base, "after a consuming 64-row launch")
    assert ops.rows_xb_launch_count() == 0
    # ... and armed through the C-ABI right before the launch, it is taken: the same bits as x_round="bf16"
    assert lib.fo_gemm_set_x_bf16(1) == 0
    got = case.run(case.x)
    assert ops.rows_xb_launch_count() == 1
    _equal(got, case.run(case.x.bfloat16().float()), "armed through the C-ABI")
    _equal(case.run(case.x), base, "the launch after it")
    assert ops.rows_xb_launch_count() == 1


def test_bad_value_is_refused_and_disarms(dev):
    from fo import _lib, ops
    lib = _lib.load()
    case = Plain(97, 2320, 4096, dev)
    base = case.run(case.x)
    assert lib.fo_gemm_set_x_bf16(1) == 0
    assert lib.fo_gemm_set_x_bf16(2) == -2 and "fo_gemm_set_x_bf16" in _lib.last_error()
    got = case.run(case.x)
    torch.cuda.synchronize()
    _equal(got, base, "after a refused fo_gemm_set_x_bf16(2)")
    assert ops.rows_xb_launch_count() == 0
    with pytest.raises(ValueError, match="x_round"):
        case.run(case.x, "fp16")
