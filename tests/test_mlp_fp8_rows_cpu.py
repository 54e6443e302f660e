"""The mlp_fp8_rows option's surface that needs no GPU: the command-line flags of bin/inference.py and bin/server.py,
and the C-ABI entry fo_gemm_w8_rows in include/fo_hip.h against fo._lib's table."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = ["--model_path", "m", "--llm_path", "l", "--input_wav", "i.wav", "--output_wav", "o.wav"]


def test_inference_flag():
    from bin.inference import get_args
    assert get_args(BASE).llm_mlp_fp8_rows == 16
    assert get_args(BASE + ["--llm_mlp_weights", "fp8", "--llm_mlp_fp8_rows", "64"]).llm_mlp_fp8_rows == 64
    with pytest.raises(SystemExit):
        get_args(BASE + ["--llm_mlp_fp8_rows", "32"])


def test_server_flag():
    from bin.server import get_parser
    p = get_parser()
    assert p.parse_args([]).llm_mlp_fp8_rows is None
    assert p.parse_args(["--llm_mlp_fp8_rows", "64"]).llm_mlp_fp8_rows == 64
    assert p.parse_args(["--llm_mlp_fp8_rows", "16"]).llm_mlp_fp8_rows == 16
    with pytest.raises(SystemExit):
        p.parse_args(["--llm_mlp_fp8_rows", "32"])


def test_header_declares_the_entry_and_the_table_matches():
    from fo import _lib
    with open(os.path.join(ROOT, "include", "fo_hip.h")) as f:
        h = f.read()
    assert re.search(r"FO_L_GEMM_W8_ROWS\s*=\s*22\b", h) and re.search(r"FO_LAUNCH_KINDS\s*=\s*24\b", h)
    m = re.search(r"\bint\s+fo_gemm_w8_rows\s*\(([^)]*)\)\s*;", h)
    assert m, "include/fo_hip.h does not declare fo_gemm_w8_rows"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "fo_gemm_w8" in v)
    assert "fo_gemm_w8_rows" in table
    assert len(table["fo_gemm_w8_rows"][1]) == nargs == len(table["fo_gemm_w8"][1])
