"""The mlp_mxfp4_rows option's surface that needs no GPU: the command-line flags of bin/inference.py and bin/server.py,
the C-ABI entries fo_gemm_w4_rows / fo_gemm_w4_rows_count in include/fo_hip.h against fo._lib's table, and the entry's
argument checks, which refuse before the library touches the device."""
import ctypes
import os
import re

import pytest

from test_quant_w4_cpu import FAKE, needs_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = ["--model_path", "m", "--llm_path", "l", "--input_wav", "i.wav", "--output_wav", "o.wav"]


def test_inference_flag():
    from bin.inference import get_args
    assert get_args(BASE).llm_mlp_mxfp4_rows == 16
    assert get_args(BASE + ["--llm_mlp_weights", "mxfp4", "--llm_mlp_mxfp4_rows", "64"]).llm_mlp_mxfp4_rows == 64
    with pytest.raises(SystemExit):
        get_args(BASE + ["--llm_mlp_mxfp4_rows", "32"])


def test_server_flag():
    from bin.server import get_parser
    p = get_parser()
    assert p.parse_args([]).llm_mlp_mxfp4_rows is None      # the config's value, else 16
    assert p.parse_args(["--llm_mlp_mxfp4_rows", "64"]).llm_mlp_mxfp4_rows == 64
    assert p.parse_args(["--llm_mlp_mxfp4_rows", "16"]).llm_mlp_mxfp4_rows == 16
    with pytest.raises(SystemExit):
        p.parse_args(["--llm_mlp_mxfp4_rows", "32"])


def test_header_declares_the_entries_and_the_table_matches():
    from fo import _lib
    with open(os.path.join(ROOT, "include", "fo_hip.h")) as f:
        h = f.read()
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "fo_gemm_w4" in v)
    m = re.search(r"\bint\s+fo_gemm_w4_rows\s*\(([^)]*)\)\s*;", h)
    assert m, "include/fo_hip.h does not declare fo_gemm_w4_rows"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert "fo_gemm_w4_rows" in table
    assert len(table["fo_gemm_w4_rows"][1]) == nargs == len(table["fo_gemm_w4"][1])
    assert re.search(r"\blong long\s+fo_gemm_w4_rows_count\s*\(\s*void\s*\)\s*;", h)
    assert table["fo_gemm_w4_rows_count"] == (ctypes.c_longlong, [])


def _rows(lib, M=32, K=128, N=64, scale=FAKE, ntiles=None, swiglu=0):
    nt = (N + 15) // 16 * (2 if swiglu else 1) if ntiles is None else ntiles
    return lib.fo_gemm_w4_rows(FAKE, K, M, K, FAKE, scale, nt, N, swiglu, FAKE, N, 0, None, 0, None, None, 0,
                               ctypes.c_float(0.0), None, None, None, None, None)


@needs_lib
def test_gemm_w4_rows_refuses_before_touching_the_device():
    from fo import _lib
    lib, err = _lib.load(), _lib.last_error
    calls = lib.fo_gemm_w4_rows_count()
    for M in (16, 65):
        assert _rows(lib, M=M) == -2 and f"M={M}" in err() and "17 <= M <= 64" in err(), err()
    assert _rows(lib, K=100) == -2 and "K=100" in err() and "multiple of 32" in err(), err()
    assert _rows(lib, scale=None) == -2 and "scale" in err(), err()
    assert _rows(lib, N=40, swiglu=1, ntiles=5) == -2 and "ntiles=5" in err() and "swiglu" in err(), err()
    assert _rows(lib, N=40, ntiles=2) == -2 and "ntiles=2" in err(), err()          # not the weight's tile count
    # a producer needs a plain launch
    assert lib.fo_gemm_w4_rows(FAKE, 128, 32, 128, FAKE, FAKE, 8, 64, 1, FAKE, 64, 0, None, 0, None, None, 0,
                               ctypes.c_float(0.0), FAKE, FAKE, FAKE, None, None) == -2 and "sout" in err(), err()
    # the down's K splits over 11 slices at 2 row blocks: no workspace, no launch
    assert _rows(lib, K=18944) == -2 and "floats needed" in err() and str(11 * 32 * 64) in err(), err()
    assert lib.fo_gemm_w4_rows_count() == calls     # a refused call is not counted


@needs_lib
def test_counters_keep_their_shape():
    from fo import ops
    lib = ops._lib.load()
    assert lib.fo_gemm_w4_counts(None, 0) == 3
    assert len(ops.LAUNCH_KINDS) == 25
    assert set(ops.w4_launch_counts()) == {"w4", "w4_xs", "w4_sk"}
    assert lib.fo_gemm_w4_rows_count() >= 0 and ops.w4_rows_launch_count() >= 0
