"""attn_weights on the host: every argument refusal of fo_gemm_w8_qkv_rope / fo_gemm_w4_qkv_rope (made before the library
touches the device, and uncounted), the C-ABI declarations, fo.quant's rope-paired packed order against a direct index
construction, the command lines' flag and the config key, and FakeQuantSource's keyword.  No GPU needed."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("FO_LIB_PATH") or os.path.join(ROOT, "freeze-omni_amd", "fo", "libfo_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libfo_hip.so not built (run __graft_entry__.build())")

FAKE = 1 << 20   # dummy device addresses: never dereferenced by a refused call
ENTRIES = ("fo_gemm_w8_qkv_rope", "fo_gemm_w4_qkv_rope")


# ------------------------------------------------------------------ the C-ABI
def test_header_declares_the_entries_and_counters():
    from fo import _lib
    txt = open(os.path.join(ROOT, "include", "fo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES + ("fo_gemm_qkv_quant_counts", "fo_gemm_qkv_quant_counts_reset"):
        m = re.search(r"int\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        args = m.group(1).strip()
        n = 0 if args in ("", "void") else len(args.split(","))
        assert n == len(_lib._SIGS[name][1]), name
    assert len(_lib._SIGS[ENTRIES[0]][1]) == 25 and _lib._SIGS[ENTRIES[0]][1] == _lib._SIGS[ENTRIES[1]][1]
    # the layout, the epilogue order and the refusals stand beside them
    doc = txt[txt.index("The fused q|k|v projection of a Qwen2 layer"):txt.index("int fo_gemm_w8_qkv_rope")]
    for word in ("h * (hd/16) + p", "tile_stride 2", "(2P, 2P + 1)", "in this order", "column scales", "rstd", "the bias",
                 "rotate_half", "slot[rr]", "[page][KVH][PS][hd]", "fo_set_kv_bf16", "M outside 1..16", "hd % 32 != 0",
                 "ntiles != N / 16", "kv_bytes not 2 or 4", "PS <= 0", "rstats without rgroups", "2 GiB"):
        assert word in doc, word


@needs_lib
def test_counter_shapes_and_policy():
    from fo import ops
    lib = ops._lib.load()
    assert lib.fo_gemm_qkv_quant_counts(None, 0) == 2
    assert tuple(ops.qkv_quant_launch_counts()) == ("w8_qkv_rope", "w4_qkv_rope") == ops.QKV_QUANT_LAUNCH_KINDS
    assert len(ops.LAUNCH_KINDS) == 25 and lib.fo_launch_counts(None, 0) == 25      # no new FoLaunchKind
    assert set(ops.ATTN_POLICY) == {"fp8", "mxfp4"}
    for fmt in ops.ATTN_POLICY:
        assert set(ops.ATTN_POLICY[fmt]) == {"qkv", "o"}
        assert all(isinstance(v, bool) for v in ops.ATTN_POLICY[fmt].values())


def _qkv(lib, entry, X=FAKE, ldx=128, M=8, K=128, q=FAKE, scale=FAKE, ntiles=None, N=None, bias=FAKE, rstats=None,
         rgroups=0, pos=FAKE, slot=FAKE, cos_t=FAKE, sin_t=FAKE, q_out=FAKE, kc=FAKE, vc=FAKE, H=2, KVH=1, hd=32, PS=16,
         kv_bytes=4):
    N = (H + 2 * KVH) * hd if N is None else N
    nt = N // 16 if ntiles is None else ntiles
    return getattr(lib, entry)(X, ldx, M, K, q, scale, nt, N, bias, rstats, rgroups, 1e-6, pos, slot, cos_t, sin_t, q_out,
                               kc, vc, H, KVH, hd, PS, kv_bytes, None)


@needs_lib
@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_before_touching_the_device(entry):
    from fo import _lib, ops
    lib, err = _lib.load(), _lib.last_error
    ops.qkv_quant_launch_counts_reset()
    ops.w4_launch_counts_reset()
    before = ops.launch_counts()

    def refused(*words, **kw):
        assert _qkv(lib, entry, **kw) == -2, kw
        msg = err()
        assert msg.startswith(entry + ":"), msg
        for w in words:
            assert w in msg, (w, msg)

    refused("M=0", M=0)
    refused("M=17", M=17)
    refused("M=-2", M=-2)
    refused("K=144", "multiple of 32", K=144, ldx=144)
    refused("hd=48", "multiple of 32", hd=48, H=2, KVH=1)          # N = 192: a whole number of tiles, hd % 32 != 0
    refused("hd=0", hd=0, N=128)
    refused("N=160", "(H + 2 KVH) * hd", N=160)                     # N != (2 + 2) * 32
    refused("N=128", "(H + 2 KVH) * hd", H=3, N=128)                # H disagrees with N
    refused("ntiles=7", ntiles=7)
    refused("ntiles=9", ntiles=9)
    refused("kv_bytes 3", kv_bytes=3)
    refused("kv_bytes 0", kv_bytes=0)
    refused("kv_bytes 8", kv_bytes=8)
    refused("PS=0", PS=0)
    refused("PS=-16", PS=-16)
    refused("NULL", X=None)
    refused("NULL", q=None)
    refused("NULL scale", scale=None)
    for name in ("pos", "slot", "cos_t", "sin_t", "q_out", "kc", "vc"):
        refused("NULL", **{name: None})
    refused("ldx=96", ldx=96)                                       # ldx < K
    refused("ldx=130", ldx=130)                                     # ldx % 4
    refused("16-byte", X=FAKE + 4)                                  # alignment
    refused("rstats without rgroups", rstats=FAKE, rgroups=0)
    # >= 2 GiB of codes: 56 KiB (FP8) / 28 KiB (MXFP4) per tile at K = 3584
    big = 40000 if entry == ENTRIES[0] else 80000
    refused("2 GiB", f"ntiles={big}", K=3584, ldx=3584, H=big // 8 - 2, KVH=1, hd=128)
    assert ops.qkv_quant_launch_counts() == {"w8_qkv_rope": 0, "w4_qkv_rope": 0}      # a refused call is not counted
    assert ops.launch_counts() == before and sum(ops.w4_launch_counts().values()) == 0


# ------------------------------------------------------------------ the rope-paired packed order
def _tile_of(n, hd):
    """The packed tile and the row within it of logical output row n."""
    h, i = divmod(n, hd)
    p, j = divmod(i, hd // 2)
    return h * (hd // 16) + p + 2 * (j // 16), j % 16


@pytest.mark.parametrize("hd", [32, 128])
def test_pack_rope_against_direct_indices(hd):
    from fo import quant
    g = torch.Generator().manual_seed(hd)
    N, K = 3 * hd, 160                                              # K % 64 == 32 and K % 128 == 32
    q8 = torch.randint(0, 256, (N, K), dtype=torch.uint8, generator=g)
    e8 = torch.randint(-20, 5, (N,), dtype=torch.int32, generator=g)
    q4 = torch.randint(0, 16, (N, K), dtype=torch.uint8, generator=g)
    e4 = torch.randint(-20, 5, (N, K // 32), dtype=torch.int32, generator=g)
    c8, s8 = quant.pack_codes_rope(q8, hd), quant.pack_scales_rope(e8, hd)
    c4, s4 = quant.pack_codes_rope_w4(q4, hd), quant.pack_scales_rope_w4(e4, hd)
    KK8, KK4 = (K + 63) // 64, (K + 127) // 128
    assert c8.numel() == N // 16 * KK8 * 1024 and s8.numel() == N
    assert c4.numel() == N // 16 * KK4 * 1024 and s4.numel() == N // 16 * KK4 * 64
    w8 = torch.zeros_like(c8).view(N // 16, KK8, 64, 16)
    w4 = torch.zeros_like(c4).view(N // 16, KK4, 64, 16)
    ws8 = torch.ones(N // 16, 16)
    ws4 = torch.full((N // 16, KK4, 16, 4), 127, dtype=torch.uint8)
    for n in range(N):
        t, r = _tile_of(n, hd)
        ws8[t, r] = 2.0 ** int(e8[n])
        for k in range(K):
            # FP8: code step k / 64, lane 16 (k % 32 / 8) + r, byte 8 (k % 64 / 32) + k % 8
            w8[t, k // 64, 16 * (k % 32 // 8) + r, 8 * (k % 64 // 32) + k % 8] = q8[n, k]
            # MXFP4: code step k / 128, lane 16 (k % 32 / 8) + r, dword k % 128 / 32, nibble k % 8 of the dword
            b = 4 * (k % 128 // 32) + (k % 8) // 2
            w4[t, k // 128, 16 * (k % 32 // 8) + r, b] |= q4[n, k] << (4 * (k % 2))
        for kb in range(K // 32):
            ws4[t, kb // 4, r, kb % 4] = int(e4[n, kb]) + 127
    assert torch.equal(c8, w8.reshape(-1)) and torch.equal(s8, ws8.reshape(-1))
    assert torch.equal(c4, w4.reshape(-1)) and torch.equal(s4, ws4.reshape(-1))
    # adjacent packed tiles (2P, 2P + 1) hold columns (i, i + hd/2) of one head
    for n in range(0, N, 7):
        if n % hd < hd // 2:
            (t0, r0), (t1, r1) = _tile_of(n, hd), _tile_of(n + hd // 2, hd)
            assert t0 % 2 == 0 and t1 == t0 + 1 and r0 == r1
    with pytest.raises(ValueError):
        quant.pack_codes_rope(q8, 48)
    with pytest.raises(ValueError):
        quant.pack_scales_rope(e8[:hd + 16], hd)


# ------------------------------------------------------------------ the flag, the config key, the source
def test_cli_flag():
    import importlib
    inf, srv = importlib.import_module("bin.inference"), importlib.import_module("bin.server")
    base = ["--model_path", "m", "--llm_path", "l", "--input_wav", "i.wav", "--output_wav", "o.wav"]
    assert inf.get_args(base).llm_attn_weights == "bf16"
    assert srv.get_parser().parse_args([]).llm_attn_weights is None      # the config's value, else bf16
    for v in ("bf16", "fp8", "mxfp4"):
        assert inf.get_args(base + ["--llm_attn_weights", v]).llm_attn_weights == v
        assert srv.get_parser().parse_args(["--llm_attn_weights", v]).llm_attn_weights == v
    for bad in ("int8", "fp4", ""):
        with pytest.raises(SystemExit):
            inf.get_args(base + ["--llm_attn_weights", bad])
        with pytest.raises(SystemExit):
            srv.get_parser().parse_args(["--llm_attn_weights", bad])
    a = inf.get_args(base + ["--llm_attn_weights", "fp8"])
    assert (a.llm_mlp_weights, a.llm_kv, a.llm_lm_head_weights) == ("bf16", "fp32", "bf16")


def test_flag_and_config_key_reach_the_engine_constructor(monkeypatch):
    import models.audioLLM as al
    import models.pipeline as pl
    seen = []

    class Engine:
        def __init__(self, *a, **kw):
            seen.append(kw)
            raise RuntimeError("stop here")

    monkeypatch.setattr(al, "FreezeOmniEngine", Engine)
    for args, want in (({"llm_attn_weights": "mxfp4"}, "mxfp4"), ({"llm_attn_weights": "fp8"}, "fp8"), ({}, "bf16"),
                       ({"llm_attn_weights": None}, "bf16")):
        with pytest.raises(RuntimeError, match="stop here"):
            pl.inferencePipeline(dict(model_path="m", llm_path="l", **args))
        assert seen[-1]["attn_weights"] == want and seen[-1]["lm_head_weights"] == "bf16"
    # the duplex server's config key travels into the pipeline's arguments
    src = open(os.path.join(ROOT, "freeze-omni_amd", "bin", "dialog_state_pred.py")).read()
    assert '"llm_attn_weights": c.get("llm_attn_weights", "bf16")' in src
    src = open(os.path.join(ROOT, "freeze-omni_amd", "bin", "server.py")).read()
    assert 'cfg["llm_attn_weights"] = getattr(args, "llm_attn_weights", None) or cfg.get("llm_attn_weights", "bf16")' in src


def test_llm_engine_validates_the_value_first():
    from fo.llm import LLMEngine
    for bad in ("int8", None, "FP8"):
        with pytest.raises(ValueError, match="attn_weights"):
            LLMEngine(None, {}, "cpu", attn_weights=bad)


def test_fake_quant_source_attn_keyword():
    from fo.weights import FakeQuantSource
    a = FakeQuantSource(object())
    assert (a.fmt, a.lm_head, a.attn) == ("fp8", None, None)
    for fmt in ("fp8", "mxfp4"):
        s = FakeQuantSource(object(), "mxfp4", lm_head="fp8", attn=fmt)
        assert (s.fmt, s.lm_head, s.attn) == ("mxfp4", "fp8", fmt)
        s = FakeQuantSource(object(), None, attn=fmt)                    # quantised projections over a bf16 MLP
        assert (s.fmt, s.lm_head, s.attn) == (None, None, fmt)
    for bad in ("bf16", "int8", True):
        with pytest.raises(ValueError):
            FakeQuantSource(object(), "fp8", attn=bad)
    with pytest.raises(ValueError):
        FakeQuantSource(object(), None)

    class Inner:
        def get(self, name, dtype=None):
            return (name, dtype)

    s = FakeQuantSource(Inner(), None, attn="fp8")
    # the biases, the MLP, the head, the embedding and the speech decoder's projections pass through
    for name in ("model.layers.0.self_attn.q_proj.bias", "model.layers.3.mlp.down_proj.weight", "lm_head.weight",
                 "model.embed_tokens.weight", "layers.0.self_attn.q_proj.weight"):
        assert s.get(name, "d") == (name, "d")
    # without the keyword the projections pass through too
    name = "model.layers.0.self_attn.o_proj.weight"
    assert FakeQuantSource(Inner(), "fp8").get(name, "d") == (name, "d")
