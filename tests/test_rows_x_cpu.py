"""llm_rows_x (bf16 GEMM inputs for the 65..128-row Qwen2 forwards) without a GPU: the format table, the
option checks of the three engines (made before any device work), the two command lines and the C-ABI arm's refusals."""
import importlib
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("FO_LIB_PATH") or os.path.join(ROOT, "freeze-omni_amd", "fo", "libfo_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libfo_hip.so not built (run __graft_entry__.build())")


def test_format_table():
    from fo.quant import FORMATS, check_format
    assert FORMATS["llm_rows_x"] == ("fp32", "bf16")
    for v in ("fp32", "bf16"):
        assert check_format("llm_rows_x", v) == v
    with pytest.raises(ValueError, match="llm_rows_x must be 'fp32' or 'bf16', got 'fp16'"):
        check_format("llm_rows_x", "fp16")


def test_engines_refuse_a_bad_value_before_any_device_work(monkeypatch):
    from fo.engine import FreezeOmniEngine
    from fo.llm import LLMEngine
    from fo.stack import DecoderStack
    words = "llm_rows_x must be 'fp32' or 'bf16', got 'fp16'"
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with pytest.raises(ValueError, match=words):
        FreezeOmniEngine("nowhere", llm_rows_x="fp16")
    with pytest.raises(ValueError, match=words):
        LLMEngine(None, {}, "cpu", rows_x="fp16")
    with pytest.raises(ValueError, match=words):
        DecoderStack(None, "model.layers.", 2, 64, 2, 2, 1e-6, True, (None, None), None, rows_x="fp16")
    # a legal value passes the checks and goes on to look for the model, with every other option beside it
    for kw in (dict(), dict(mlp_weights="mxfp4", lm_head_weights="mxfp6", attn_weights="fp8", llm_kv="e4m3")):
        with pytest.raises(Exception) as ei:
            FreezeOmniEngine("nowhere", llm_rows_x="bf16", **kw)
        assert "must be" not in str(ei.value)
    # a stack with no layers needs no device: the option is kept as given
    assert DecoderStack(None, "model.layers.", 0, 64, 2, 2, 1e-6, True, (None, None), None, rows_x="bf16").rows_x == "bf16"
    assert DecoderStack(None, "model.layers.", 0, 64, 2, 2, 1e-6, True, (None, None), None).rows_x == "fp32"


def test_command_lines():
    from fo.quant import FORMATS
    inf, srv = importlib.import_module("bin.inference"), importlib.import_module("bin.server")
    base = ["--model_path", "m", "--llm_path", "l", "--input_wav", "i", "--output_wav", "o"]
    assert inf.get_args(base).llm_rows_x == "fp32"
    assert inf.get_args(base + ["--llm_rows_x", "bf16"]).llm_rows_x == "bf16"
    # (the server's options default to None: the YAML's value, else the engine's default -- fp32 -- decides)
    assert (srv.get_parser().parse_args([]).llm_rows_x or "fp32") == "fp32"
    assert srv.get_parser().parse_args(["--llm_rows_x", "bf16"]).llm_rows_x == "bf16"
    for v in FORMATS["llm_rows_x"]:
        assert srv.get_parser().parse_args(["--llm_rows_x", v]).llm_rows_x == v
    for bad in ("fp16", "e4m3"):
        with pytest.raises(SystemExit):
            inf.get_args(base + ["--llm_rows_x", bad])
        with pytest.raises(SystemExit):
            srv.get_parser().parse_args(["--llm_rows_x", bad])


def test_x_round_is_checked_by_name():
    from fo import ops
    assert ops.X_ROUNDS == (None, "bf16")
    with pytest.raises(ValueError, match="x_round must be one of"):
        ops._packed(None, None, x_round="fp16")


@needs_lib
def test_arm_refuses_other_values_by_name():
    from fo import _lib, ops
    lib = _lib.load()
    ops.rows_xb_launch_count_reset()
    for v in (2, -1):
        assert lib.fo_gemm_set_x_bf16(v) == -2, v
        assert "fo_gemm_set_x_bf16" in _lib.last_error() and str(v) in _lib.last_error(), _lib.last_error()
    assert lib.fo_gemm_set_x_bf16(1) == 0 and lib.fo_gemm_set_x_bf16(0) == 0
    assert ops.rows_xb_launch_count() == 0
    ops.rows_xb_launch_count_reset()
    assert lib.fo_gemm_rows_xb_count() == 0
