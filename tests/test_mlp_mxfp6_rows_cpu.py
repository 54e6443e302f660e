"""The mlp_mxfp6_rows option's surface that needs no GPU: the command-line flags of bin/inference.py and bin/server.py,
the C-ABI entries fo_gemm_w6_rows / fo_gemm_w6_rows_count in include/fo_hip.h against fo._lib's table, the entry's
argument checks, which refuse before the library touches the device, and the engine's option checks."""
import ctypes
import os
import re

import pytest
import torch

from test_quant_w6_cpu import FAKE, needs_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = ["--model_path", "m", "--llm_path", "l", "--input_wav", "i.wav", "--output_wav", "o.wav"]


def test_inference_flag():
    from bin.inference import get_args
    assert get_args(BASE).llm_mlp_mxfp6_rows == 16
    assert get_args(BASE + ["--llm_mlp_weights", "mxfp6", "--llm_mlp_mxfp6_rows", "64"]).llm_mlp_mxfp6_rows == 64
    with pytest.raises(SystemExit):
        get_args(BASE + ["--llm_mlp_mxfp6_rows", "32"])


def test_server_flag():
    from bin.server import get_parser
    p = get_parser()
    assert p.parse_args([]).llm_mlp_mxfp6_rows is None      # the config's value, else 16
    assert p.parse_args(["--llm_mlp_mxfp6_rows", "64"]).llm_mlp_mxfp6_rows == 64
    assert p.parse_args(["--llm_mlp_mxfp6_rows", "16"]).llm_mlp_mxfp6_rows == 16
    with pytest.raises(SystemExit):
        p.parse_args(["--llm_mlp_mxfp6_rows", "32"])


def test_header_declares_the_entries_and_the_table_matches():
    from fo import _lib
    with open(os.path.join(ROOT, "include", "fo_hip.h")) as f:
        h = f.read()
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "fo_gemm_w6" in v)
    m = re.search(r"\bint\s+fo_gemm_w6_rows\s*\(([^)]*)\)\s*;", h)
    assert m, "include/fo_hip.h does not declare fo_gemm_w6_rows"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    m6 = re.search(r"\bint\s+fo_gemm_w6\s*\(([^)]*)\)\s*;", h)
    assert "fo_gemm_w6_rows" in table
    assert len(table["fo_gemm_w6_rows"][1]) == nargs == len(table["fo_gemm_w6"][1])
    assert nargs == len([a for a in m6.group(1).split(",") if a.strip()])
    assert re.search(r"\blong long\s+fo_gemm_w6_rows_count\s*\(\s*void\s*\)\s*;", h)
    assert table["fo_gemm_w6_rows_count"] == (ctypes.c_longlong, [])


def test_format_table_and_layer_policy():
    from fo import ops
    fm = ops.QUANT_FORMATS["mxfp6"]
    assert fm.stream_rows == (16, 64) and fm.rows == {64: "fo_gemm_w6_rows"}
    assert set(ops.W6_ROWS_POLICY) <= {"gate_up", "down"}
    assert all(set(v) <= {2, 3, 4} for v in ops.W6_ROWS_POLICY.values())
    # the row policy reaches a layer only when it is built with the band; FP8 and MXFP4 carry theirs at any stream_rows
    for gemm in ("gate_up", "down"):
        assert ops._policy("mxfp6", gemm, 3584) == (bool(ops.W6_POLICY[gemm]), ())
        assert ops._policy("mxfp6", gemm, 3584, 64) == (bool(ops.W6_POLICY[gemm]),
                                                       tuple(ops.W6_ROWS_POLICY.get(gemm, ())))
        assert ops._policy("mxfp4", gemm, 3584)[1] == ops._policy("mxfp4", gemm, 3584, 64)[1] == ops.W4_ROWS_POLICY[gemm]
        assert ops._policy("fp8", gemm, 3584)[1] == ops._policy("fp8", gemm, 3584, 128)[1] == ops.W8_ROWS_POLICY[gemm]
    assert ops._policy("mxfp6", "head", 3584, 64)[1] == ()


def _rows(lib, M=32, K=128, N=64, X=FAKE, Q=FAKE, Y=FAKE, scale=FAKE, ntiles=None, swiglu=0, ldx=None, ldy=None):
    nt = (N + 15) // 16 * (2 if swiglu else 1) if ntiles is None else ntiles
    return lib.fo_gemm_w6_rows(X, K if ldx is None else ldx, M, K, Q, scale, nt, N, swiglu, Y, N if ldy is None else ldy,
                               0, None, 0, None, None, 0, ctypes.c_float(0.0), None, None, None, None, None)


@needs_lib
def test_gemm_w6_rows_refuses_before_touching_the_device():
    from fo import _lib, ops
    lib, err = _lib.load(), _lib.last_error
    calls, forms = lib.fo_gemm_w6_rows_count(), ops.w6_launch_counts()
    for M in (16, 65):
        assert _rows(lib, M=M) == -2 and f"M={M}" in err() and "17 <= M <= 64" in err(), err()
        assert "fo_gemm_w6_rows:" in err(), err()
    assert _rows(lib, K=100) == -2 and "K=100" in err() and "multiple of 32" in err(), err()
    for null in ("X", "Q", "Y"):
        assert _rows(lib, **{null: None}) == -2 and "NULL" in err() and "fo_gemm_w6_rows:" in err(), err()
    assert _rows(lib, scale=None) == -2 and "scale" in err(), err()
    assert _rows(lib, ldx=96) == -2 and "ldx=96" in err(), err()
    assert _rows(lib, ldx=130) == -2 and "ldx" in err(), err()               # ldx % 4 != 0
    assert _rows(lib, X=FAKE + 4) == -2 and "alignment" in err(), err()
    assert _rows(lib, ldy=48) == -2 and "ldy=48" in err(), err()
    assert _rows(lib, N=40, swiglu=1, ntiles=5) == -2 and "ntiles=5" in err() and "swiglu" in err(), err()
    assert _rows(lib, N=40, ntiles=2) == -2 and "ntiles=2" in err(), err()          # not the weight's tile count
    # a producer needs a plain launch
    assert lib.fo_gemm_w6_rows(FAKE, 128, 32, 128, FAKE, FAKE, 8, 64, 1, FAKE, 64, 0, None, 0, None, None, 0,
                               ctypes.c_float(0.0), FAKE, FAKE, FAKE, None, None) == -2 and "sout" in err(), err()
    # codes of 2 GiB or more
    assert _rows(lib, N=16 * 1400000) == -2 and "2 GiB" in err(), err()
    # the down's K is 148 code steps: 22 slices of 7 at 2 row blocks (7 waves x 1 code step): no workspace, no launch
    assert _rows(lib, K=18944) == -2 and "floats needed" in err() and f"({22 * 32 * 64} floats needed" in err(), err()
    # ... 19 slices of 8 at 3 row blocks (plain: 8 waves), 25 of 6 at 4
    assert _rows(lib, M=48, K=18944) == -2 and f"({19 * 48 * 64} floats needed" in err(), err()
    assert _rows(lib, M=64, K=18944) == -2 and f"({25 * 64 * 64} floats needed" in err(), err()
    assert lib.fo_gemm_w6_rows_count() == calls     # a refused call is not counted
    assert ops.w6_launch_counts() == forms


@needs_lib
def test_counters_keep_their_shape():
    from fo import ops
    lib = ops._lib.load()
    assert lib.fo_gemm_w6_counts(None, 0) == 4
    assert len(ops.LAUNCH_KINDS) == 25
    assert tuple(ops.w6_launch_counts()) == ("w6", "w6_xs", "w6_sk", "w6_head")
    assert lib.fo_gemm_w6_rows_count() >= 0 and ops.w6_rows_launch_count() >= 0


def test_engine_option_checks(monkeypatch):
    """The option checks come before anything touches a device or a model directory."""
    from fo.engine import FreezeOmniEngine
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    for fmt in ("fp8", "bf16", "mxfp4"):
        with pytest.raises(ValueError, match="mlp_mxfp6_rows=64 needs mlp_weights='mxfp6'"):
            FreezeOmniEngine("nowhere", mlp_weights=fmt, mlp_mxfp6_rows=64)
    with pytest.raises(ValueError, match="mlp_mxfp6_rows must be"):
        FreezeOmniEngine("nowhere", mlp_weights="mxfp6", mlp_mxfp6_rows=32)
    # the older options keep their messages
    with pytest.raises(ValueError, match="mlp_fp8_rows=64 needs mlp_weights='fp8'"):
        FreezeOmniEngine("nowhere", mlp_weights="mxfp6", mlp_fp8_rows=64)
    with pytest.raises(ValueError, match="mlp_mxfp4_rows=64 needs mlp_weights='mxfp4'"):
        FreezeOmniEngine("nowhere", mlp_weights="mxfp6", mlp_mxfp4_rows=64)
    # the legal combination passes the checks and goes on to look for the model
    with pytest.raises(Exception) as ei:
        FreezeOmniEngine("nowhere", mlp_weights="mxfp6", mlp_mxfp6_rows=64)
    assert "must be" not in str(ei.value) and "needs mlp_weights" not in str(ei.value)
