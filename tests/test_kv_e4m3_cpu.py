"""The FP8 (e4m3) paged KV cache of the Qwen2 stack (llm_kv="e4m3") without a GPU: the CPU model
fo.quant.quantize_kv_rows, the option's spelling through the formats table, the command lines and the engine, the
pool's storage, and the host-side refusals of fo_kv8_append / fo_attention_kv8 (made before the entry's first HIP call,
so the made-up addresses are never dereferenced)."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("FO_LIB_PATH") or os.path.join(ROOT, "freeze-omni_amd", "fo", "libfo_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libfo_hip.so not built (run __graft_entry__.build())")
FP8 = torch.float8_e4m3fn


# ---------------------------------------------------------------- the model
def test_quantize_kv_rows_properties():
    from fo.quant import quantize_kv_rows, quantize_rows_e4m3
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 4, 128, generator=g) * torch.ldexp(torch.ones(5, 4, 1), torch.randint(-6, 3, (5, 4, 1), generator=g))
    q, e, img = quantize_kv_rows(x)
    assert q.dtype == torch.uint8 and q.shape == x.shape
    assert e.dtype == torch.int32 and e.shape == x.shape[:-1]
    assert img.dtype == torch.bfloat16 and img.shape == x.shape
    # the image is exactly code * 2^e, and exactly a bf16 value (the float64 product survives the round trip)
    exact = q.view(FP8).double() * torch.ldexp(torch.ones(5, 4, 1, dtype=torch.float64), e[..., None])
    assert torch.equal(img.double(), exact)
    assert float(q.view(FP8).float().abs().max()) <= 448
    # the scaled row maximum lies in (224, 448] (e is the smallest exponent that fits) and rounds within [224, 448]
    top = q.view(FP8).float().abs().amax(-1)
    assert float(top.min()) >= 224 and float(top.max()) <= 448
    # it is the row quantiser over the flattened rows
    q2, e2, img2 = quantize_rows_e4m3(x.reshape(-1, 128))
    assert torch.equal(q.reshape(-1, 128), q2) and torch.equal(e.reshape(-1), e2)
    assert torch.equal(img.reshape(-1, 128).view(torch.int16), img2.view(torch.int16))
    # per-element error of the model on random rows (the issue's 2.7 %), and idempotence on its own image
    rel = float((img.double() - x.double()).norm() / x.double().norm())
    assert 0.015 < rel < 0.04, rel
    assert torch.equal(quantize_kv_rows(img.float())[2].view(torch.int16), img.view(torch.int16))


def test_quantize_kv_rows_exponent_boundaries():
    from fo.quant import quantize_kv_rows

    def e_of(amax, hd=32):
        row = torch.zeros(hd)
        row[3] = -amax
        q, e, img = quantize_kv_rows(row[None])
        return int(e[0]), float(q.view(FP8)[0, 3].float()), float(img[0, 3])

    assert e_of(0.0)[0] == 0                                  # all-zero row
    assert quantize_kv_rows(torch.zeros(2, 64))[0].eq(0).all()
    assert e_of(448.0) == (0, -448.0, -448.0)                 # 448 = 1.75 * 2^8 fits at e = 0
    up = float(torch.nextafter(torch.tensor(448.0), torch.tensor(1e9)))
    assert e_of(up) == (1, -224.0, -448.0)                    # one ulp above takes the next exponent
    for k in (-20, -3, 0, 5):
        assert e_of(1.75 * 2.0 ** k)[0] == k - 8              # amax = 1.75 * 2^k: e = k - 8, the code is 448
        assert e_of(1.75 * 2.0 ** k)[1] == -448.0
        assert e_of(float(torch.nextafter(torch.tensor(1.75 * 2.0 ** k), torch.tensor(1e9))))[0] == k - 7
        assert e_of(2.0 ** k) == (k - 8, -256.0, -(2.0 ** k))
    assert e_of(2.0 ** -140)[0] == -126                       # clamped: 2^e stays a normal float


def test_quantize_kv_rows_non_finite_elements_become_nan_codes():
    from fo.quant import quantize_kv_rows
    row = torch.tensor([1.0, float("nan"), -3.5, float("inf"), float("-inf"), 0.25] + [0.0] * 26)
    q, e, img = quantize_kv_rows(row[None])
    assert int(e[0]) == 1 - 8                                 # the largest finite magnitude, 3.5 = 1.75 * 2
    assert [int(c) & 0x7F for c in q[0, [1, 3, 4]]] == [0x7F] * 3 and int(q[0, 4]) == 0xFF
    assert torch.isnan(q.view(FP8)[0, [1, 3, 4]].float()).all() and torch.isnan(img[0, [1, 3, 4]].float()).all()
    assert img[0, [0, 2, 5]].float().tolist() == [1.0, -3.5, 0.25]


# ---------------------------------------------------------------- the option
def test_format_table_and_command_lines():
    import importlib
    from fo.quant import FORMATS, check_format
    assert FORMATS["llm_kv"] == ("fp32", "bf16", "e4m3") and FORMATS["llm_kv"][-1] == "e4m3"
    assert check_format("llm_kv", "e4m3") == "e4m3"
    with pytest.raises(ValueError, match="llm_kv must be 'fp32', 'bf16' or 'e4m3', got 'fp8'"):
        check_format("llm_kv", "fp8")
    inf, srv = importlib.import_module("bin.inference"), importlib.import_module("bin.server")
    base = ["--model_path", "m", "--llm_path", "l", "--input_wav", "i.wav", "--output_wav", "o.wav"]
    assert inf.get_args(base).llm_kv == "fp32"
    assert inf.get_args(base + ["--llm_kv", "e4m3"]).llm_kv == "e4m3"
    assert srv.get_parser().parse_args(["--llm_kv", "e4m3"]).llm_kv == "e4m3"
    for bad in ("fp8", "fp16"):
        with pytest.raises(SystemExit):
            inf.get_args(base + ["--llm_kv", bad])
        with pytest.raises(SystemExit):
            srv.get_parser().parse_args(["--llm_kv", bad])


def test_engine_option_checks(monkeypatch):
    """The option checks come before anything touches a device or a model directory."""
    from fo.engine import FreezeOmniEngine
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with pytest.raises(ValueError, match="llm_kv must be 'fp32', 'bf16' or 'e4m3', got 'fp8'"):
        FreezeOmniEngine("nowhere", llm_kv="fp8")
    with pytest.raises(ValueError, match="mlp_fp8_rows=64 needs mlp_weights='fp8'"):
        FreezeOmniEngine("nowhere", llm_kv="e4m3", mlp_weights="mxfp4", mlp_fp8_rows=64)
    # legal combinations with the weight options pass the checks and go on to look for the model
    for kw in (dict(), dict(mlp_weights="mxfp4", lm_head_weights="mxfp6", attn_weights="fp8")):
        with pytest.raises(Exception) as ei:
            FreezeOmniEngine("nowhere", llm_kv="e4m3", **kw)
        assert "must be" not in str(ei.value) and "needs mlp_weights" not in str(ei.value)


def test_llm_engine_refuses_other_spellings():
    from fo.llm import LLMEngine
    with pytest.raises(ValueError, match='kv_dtype must be "fp32", "bf16" or "e4m3", got \'fp8\''):
        LLMEngine(None, {}, "cpu", kv_dtype="fp8")


# ---------------------------------------------------------------- the pool
def test_pool_storage():
    from fo.kv import KVPool, KVSeq
    L, KVH, hd, pages, PS = 3, 4, 128, 6, 16
    p = KVPool(L, KVH, hd, pages, PS, "cpu", dtype=FP8)
    assert p.fp8 and p.k.dtype == p.v.dtype == FP8 and p.k.element_size() == 1
    assert p.k.shape == p.v.shape == (L, pages, KVH, PS, hd)
    assert p.ks.dtype == p.vs.dtype == torch.float32 and p.ks.shape == p.vs.shape == (L, pages, KVH, PS)
    assert p.bytes_per_token == L * KVH * (hd + 4) * 2
    # Qwen2-7B: 28 layers x 4 kv heads of 128
    assert KVPool(28, 4, 128, 1, 16, "cpu", dtype=FP8).bytes_per_token == 29568
    for dt, b in ((torch.float32, 114688), (torch.bfloat16, 57344)):
        q = KVPool(28, 4, 128, 1, 16, "cpu", dtype=dt)
        assert q.bytes_per_token == b and q.ks is None and q.vs is None and not q.fp8
    with pytest.raises(ValueError, match="KVPool dtype"):
        KVPool(1, 1, 32, 1, 16, "cpu", dtype=torch.float16)
    with pytest.raises(ValueError, match="KVPool dtype"):
        KVPool(1, 1, 32, 1, 16, "cpu", dtype=torch.float8_e5m2)
    # copy_page copies codes and scales, of every layer, and nothing else
    g = torch.Generator().manual_seed(1)
    for t in (p.k, p.v):
        t.view(torch.uint8).copy_(torch.randint(0, 256, t.shape, generator=g, dtype=torch.uint8))
    for t in (p.ks, p.vs):
        t.copy_(torch.rand(t.shape, generator=g))
    before = [t.clone() for t in (p.k.view(torch.uint8), p.v.view(torch.uint8), p.ks, p.vs)]
    p.copy_page(2, 5)
    for t, b in zip((p.k.view(torch.uint8), p.v.view(torch.uint8), p.ks, p.vs), before):
        assert torch.equal(t[:, 5], b[:, 2]) and not torch.equal(b[:, 5], b[:, 2])
        keep = [i for i in range(pages) if i != 5]
        assert torch.equal(t[:, keep], b[:, keep])
    # copy-on-write through a fork: the child's private tail page carries the parent's scales
    a = KVSeq(p)
    a.reserve(20)
    a.length = 20
    c = a.fork()
    c.reserve(21)
    assert c.pages[0] == a.pages[0] and c.pages[1] != a.pages[1]
    assert torch.equal(p.ks[:, c.pages[1]], p.ks[:, a.pages[1]]) and torch.equal(p.vs[:, c.pages[1]], p.vs[:, a.pages[1]])
    assert torch.equal(p.k.view(torch.uint8)[:, c.pages[1]], p.k.view(torch.uint8)[:, a.pages[1]])


def test_ops_wrappers_check_the_tensors():
    from fo import ops
    from fo.kv import KVPool
    p8, p16 = KVPool(1, 2, 32, 2, 16, "cpu", dtype=FP8), KVPool(1, 2, 32, 2, 16, "cpu", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="both be fp32 or both bf16"):
        ops.kv_bytes(p8.k[0], p8.v[0])                       # the codes never reach a *_kv entry
    assert ops.kv_bytes(p16.k[0], p16.v[0]) == 2
    st = torch.zeros(1, 2, 8, 32)
    sl = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(ValueError, match="e4m3fn codes with fp32 scales"):
        ops.kv8_append(st, st, 8, sl, p16.k[0], p8.ks[0], p16.v[0], p8.vs[0], 16)
    with pytest.raises(ValueError, match="one per row"):
        ops.kv8_append(st, st, 8, sl, p8.k[0], p8.ks[0][:1], p8.v[0], p8.vs[0], 16)
    with pytest.raises(ValueError, match="kscale and vscale come together"):
        ops.attention(st, 1, None, 1, 1, sl, sl.view(1, -1), 16, p8.k[0], p8.v[0], 2, 2, 32, 1.0, 1, None, None, st,
                      kscale=p8.ks[0])


# ---------------------------------------------------------------- the C-ABI
Q, NVIS, BT, KC, VC, KS, VS, OUT, ITEMS, TK, PML, PO, STK, STV, SLOT = (0x100000 * i for i in range(1, 16))


def _append(**kw):
    a = dict(k_stage=STK, v_stage=STV, T=8, KVH=4, hd=128, stage_rows=8, slot=SLOT, PS=16, kc=KC, ks=KS, vc=VC, vs=VS,
             stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return tuple(a.values())


def _attn(**kw):
    """A launchable Qwen2-geometry call (2 tokens x 7 query heads per kv head, ticketed splits of 128 keys)."""
    a = dict(q=Q, T=4, items=ITEMS, n_items=2, max_rows=14, tok_nvis=NVIS, block_table=BT, maxb=20, PS=16, kc=KC, vc=VC,
             H=28, KVH=4, hd=128, scale=0.1, nsplit=4, part_ml=PML, part_o=PO, out=OUT, tickets=TK, keys_per_split=128,
             ks=KS, vs=VS, stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return tuple(a.values())


def _refused(entry, args, words):
    from fo import _lib, ops
    before = ops.launch_counts()
    rc = getattr(_lib.load(), entry)(*args)
    msg = _lib.last_error()
    assert rc == -2, (rc, msg)
    assert msg.startswith(entry + ": ") and words in msg, msg
    assert ops.launch_counts() == before
    assert not any(ops.kv8_launch_counts().values())


APPEND_REFUSALS = [
    ("null-kc", dict(kc=None), "NULL codes or scales"),
    ("null-vc", dict(vc=None), "NULL codes or scales"),
    ("null-ks", dict(ks=None), "NULL codes or scales"),
    ("null-vs", dict(vs=None), "NULL codes or scales"),
    ("null-stage", dict(v_stage=None), "NULL staged rows or slot table"),
    ("null-slot", dict(slot=None), "NULL staged rows or slot table"),
    ("hd-96", dict(hd=96), "head_dim 96 unsupported"),
    ("hd-256", dict(hd=256), "head_dim 256 unsupported"),
    ("PS-0", dict(PS=0), "page size 0"),
    ("PS-neg", dict(PS=-16), "page size -16"),
    ("T-0", dict(T=0), "T=0 outside 1..8 stage rows"),
    ("T-past-stage", dict(T=9), "T=9 outside 1..8 stage rows"),
]
ATTN_REFUSALS = [
    ("null-kc", dict(kc=None), "NULL codes or scales"),
    ("null-vc", dict(vc=None), "NULL codes or scales"),
    ("null-ks", dict(ks=None), "NULL codes or scales"),
    ("null-vs", dict(vs=None), "NULL codes or scales"),
    ("hd-96", dict(hd=96), "head_dim 96 unsupported"),
    ("PS-0", dict(PS=0), "page size 0"),
    ("two-wave", dict(keys_per_split=32), "2-wave form"),
    ("single-row-decode", dict(H=4, KVH=4, hd=64, max_rows=1, T=2, items=None), "single-row decode form"),
]


@needs_lib
@pytest.mark.parametrize("case", APPEND_REFUSALS, ids=[c[0] for c in APPEND_REFUSALS])
def test_kv8_append_refuses_before_touching_the_device(case):
    from fo import ops
    ops.kv8_launch_counts_reset()
    _refused("fo_kv8_append", _append(**case[1]), case[2])


@needs_lib
@pytest.mark.parametrize("case", ATTN_REFUSALS, ids=[c[0] for c in ATTN_REFUSALS])
def test_attention_kv8_refuses_before_touching_the_device(case):
    from fo import ops
    ops.kv8_launch_counts_reset()
    _refused("fo_attention_kv8", _attn(**case[1]), case[2])


@needs_lib
def test_attention_kv8_refuses_traced_launches():
    from fo import _lib, ops
    lib = _lib.load()
    ops.kv8_launch_counts_reset()
    assert lib.fo_attention_set_trace(0x7000000) == 0
    try:
        _refused("fo_attention_kv8", _attn(), "traced launches")
    finally:
        assert lib.fo_attention_set_trace(None) == 0


@needs_lib
def test_kv_entries_still_take_only_fp32_and_bf16():
    """fo_attention_kv keeps refusing every kv_bytes but 4 and 2 -- 1 included: the codes come with their scales."""
    from fo import _lib, ops
    lib = _lib.load()
    ops.launch_counts_reset()
    for kvb in (1, 0, 3, 8):
        rc = lib.fo_attention_kv(*_attn()[:-3], kvb, None)
        assert rc == -2 and f"fo_attention: kv_bytes {kvb}" in _lib.last_error(), _lib.last_error()
    assert not any(ops.launch_counts().values())


@needs_lib
def test_kv8_counters_are_their_own():
    from fo import _lib, ops
    lib = _lib.load()
    assert tuple(ops.kv8_launch_counts()) == ops.KV8_LAUNCH_KINDS == ("kv8_append", "kv8_attention")
    ops.kv8_launch_counts_reset()
    assert ops.kv8_launch_counts() == {"kv8_append": 0, "kv8_attention": 0}
    # the existing counters keep their shape: no FoLaunchKind was added
    assert (len(ops.LAUNCH_KINDS), lib.fo_launch_counts(None, 0)) == (25, 25)
    assert lib.fo_gemm_w6_counts(None, 0) == 4
    txt = open(os.path.join(ROOT, "include", "fo_hip.h")).read()
    for name in ("fo_kv8_append", "fo_attention_kv8", "fo_kv8_counts", "fo_kv8_counts_reset"):
        assert name + "(" in txt and name in _lib._SIGS and hasattr(lib, name), name
