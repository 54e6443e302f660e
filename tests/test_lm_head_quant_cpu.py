"""lm_head_weights on the host: the command lines' flag, the C-ABI declarations of fo_gemm_w8_head / fo_gemm_w4_head and
their counter pair, every argument refusal (made before the library touches the device, and uncounted), and
FakeQuantSource's keyword.  No GPU needed."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("FO_LIB_PATH") or os.path.join(ROOT, "freeze-omni_amd", "fo", "libfo_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libfo_hip.so not built (run __graft_entry__.build())")

FAKE = 1 << 20   # dummy device addresses: never dereferenced by a refused call
K = 3584


def test_cli_flag():
    import importlib
    inf, srv = importlib.import_module("bin.inference"), importlib.import_module("bin.server")
    base = ["--model_path", "m", "--llm_path", "l", "--input_wav", "i.wav", "--output_wav", "o.wav"]
    assert inf.get_args(base).llm_lm_head_weights == "bf16"
    assert srv.get_parser().parse_args([]).llm_lm_head_weights is None      # the config's value, else bf16
    for v in ("bf16", "fp8", "mxfp4"):
        assert inf.get_args(base + ["--llm_lm_head_weights", v]).llm_lm_head_weights == v
        assert srv.get_parser().parse_args(["--llm_lm_head_weights", v]).llm_lm_head_weights == v
    for bad in ("int8", "fp4", ""):
        with pytest.raises(SystemExit):
            inf.get_args(base + ["--llm_lm_head_weights", bad])
        with pytest.raises(SystemExit):
            srv.get_parser().parse_args(["--llm_lm_head_weights", bad])
    # the other options keep their defaults beside it
    a = inf.get_args(base + ["--llm_lm_head_weights", "fp8"])
    assert (a.llm_mlp_weights, a.llm_kv) == ("bf16", "fp32")


def test_header_declares_the_entries_and_counters():
    from fo import _lib
    txt = open(os.path.join(ROOT, "include", "fo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("fo_gemm_w8_head", "fo_gemm_w4_head", "fo_gemm_head_counts", "fo_gemm_head_counts_reset"):
        m = re.search(r"int\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        args = m.group(1).strip()
        n = 0 if args in ("", "void") else len(args.split(","))
        assert n == len(_lib._SIGS[name][1]), name
    assert len(_lib._SIGS["fo_gemm_w8_head"][1]) == 11          # X, ldx, M, K, q, scale, ntiles, N, Y, ldy, stream
    assert _lib._SIGS["fo_gemm_w8_head"][1] == _lib._SIGS["fo_gemm_w4_head"][1]
    # the layout text stands beside them
    doc = txt[txt.index("The Qwen2 output head"):txt.index("int fo_gemm_w8_head")]
    for word in ("[tile][56][64 lanes][16 bytes]", "[tile][28][64 lanes][16 bytes]", "[tile][28][16 rows][4]",
                 "K != 3584", "ntiles != ceil(N/16)"):
        assert word in doc, word


@needs_lib
def test_counter_shapes():
    from fo import ops
    lib = ops._lib.load()
    assert lib.fo_gemm_head_counts(None, 0) == 2
    assert tuple(ops.head_launch_counts()) == ("w8_head", "w4_head") == ops.HEAD_LAUNCH_KINDS
    assert len(ops.LAUNCH_KINDS) == 25 and lib.fo_launch_counts(None, 0) == 25
    assert lib.fo_gemm_w4_counts(None, 0) == 3
    assert set(ops.HEAD_POLICY) == {"fp8", "mxfp4"} and all(isinstance(v, bool) for v in ops.HEAD_POLICY.values())
    # the head has no entry in the row-stream policies
    assert set(ops.W8_ROWS_POLICY) == {"gate_up", "down"} and set(ops.W4_ROWS_POLICY) == {"gate_up", "down"}


def _head(lib, entry, X=FAKE, ldx=K, M=8, k=K, q=FAKE, scale=FAKE, ntiles=None, N=160, Y=FAKE, ldy=None):
    nt = (N + 15) // 16 if ntiles is None else ntiles
    return getattr(lib, entry)(X, ldx, M, k, q, scale, nt, N, Y, N if ldy is None else ldy, None)


@needs_lib
@pytest.mark.parametrize("entry", ["fo_gemm_w8_head", "fo_gemm_w4_head"])
def test_refusals_before_touching_the_device(entry):
    from fo import _lib, ops
    lib, err = _lib.load(), _lib.last_error
    ops.head_launch_counts_reset()
    ops.w4_launch_counts_reset()
    before = ops.launch_counts()

    def refused(*words, **kw):
        assert _head(lib, entry, **kw) == -2, kw
        msg = err()
        assert msg.startswith(entry + ":"), msg
        for w in words:
            assert w in msg, (w, msg)

    refused("M=0", M=0)
    refused("M=17", M=17)
    refused("M=-3", M=-3)
    refused("K=128", "3584", k=128, ldx=128)                 # a multiple of 32 that the form is not compiled for
    refused("K=7168", "3584", k=7168, ldx=7168)
    refused("K=3600", "multiple of 32", k=3600, ldx=3600)
    refused("NULL X", X=None)
    refused("NULL X", q=None)
    refused("NULL X", Y=None)
    refused("NULL scale", scale=None)
    refused("ldx=3580", ldx=3580)                            # ldx < K
    refused("ldx=3586", ldx=3586)                            # ldx % 4
    refused("16-byte", X=FAKE + 4)                           # alignment
    refused("ldy=159", "N=160", ldy=159)
    refused("ntiles=9", "N=160", ntiles=9)
    refused("ntiles=11", "N=160", ntiles=11)
    refused("ntiles=5", "N=144", N=144, ntiles=5)
    big = 16 * (40000 if entry == "fo_gemm_w8_head" else 80000)   # >= 2 GiB of codes at 56 / 28 KiB per tile
    refused("2 GiB", f"ntiles={big // 16}", N=big)
    assert ops.head_launch_counts() == {"w8_head": 0, "w4_head": 0}     # a refused call is not counted
    assert ops.launch_counts() == before and sum(ops.w4_launch_counts().values()) == 0


def test_fake_quant_source_existing_forms_are_unchanged():
    from fo.weights import FakeQuantSource
    a, b = FakeQuantSource(object()), FakeQuantSource(object(), "mxfp4")
    assert (a.fmt, a.lm_head) == ("fp8", None) and (b.fmt, b.lm_head) == ("mxfp4", None)
    with pytest.raises(ValueError):
        FakeQuantSource(object(), "int8")
    with pytest.raises(ValueError):
        FakeQuantSource(object(), None)                      # no MLP format and no head: nothing to serve

    class Inner:
        def __contains__(self, name):
            return True

        def get(self, name, dtype=None):
            return (name, dtype)

    # without the keyword lm_head.weight passes through untouched, as every non-MLP name does
    assert FakeQuantSource(Inner()).get("lm_head.weight", "d") == ("lm_head.weight", "d")
    assert FakeQuantSource(Inner(), "mxfp4").get("model.embed_tokens.weight", "d") == ("model.embed_tokens.weight", "d")


def test_fake_quant_source_lm_head_keyword():
    from fo.weights import FakeQuantSource
    for fmt in ("fp8", "mxfp4"):
        s = FakeQuantSource(object(), "fp8", lm_head=fmt)
        assert (s.fmt, s.lm_head) == ("fp8", fmt)
        s = FakeQuantSource(object(), None, lm_head=fmt)    # a quantised head over a bf16 MLP
        assert (s.fmt, s.lm_head) == (None, fmt)
    for bad in ("bf16", "int8", True):
        with pytest.raises(ValueError):
            FakeQuantSource(object(), "fp8", lm_head=bad)

    class Inner:
        def get(self, name, dtype=None):
            return (name, dtype)

    s = FakeQuantSource(Inner(), None, lm_head="fp8")
    # the embedding is never quantised, and with fmt=None neither is the MLP
    for name in ("model.embed_tokens.weight", "model.layers.0.mlp.down_proj.weight", "model.norm.weight"):
        assert s.get(name, "d") == (name, "d")
