"""mlp_fp8_rows=128's surface that needs no GPU: the command-line flags of bin/inference.py and bin/server.py, the C-ABI
entry fo_gemm_w8_rows128 in include/fo_hip.h against fo._lib's table, and the launch kinds against ops.LAUNCH_KINDS."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = ["--model_path", "m", "--llm_path", "l", "--input_wav", "i.wav", "--output_wav", "o.wav"]


def _header():
    with open(os.path.join(ROOT, "include", "fo_hip.h")) as f:
        return f.read()


def test_inference_flag():
    from bin.inference import get_args
    assert get_args(BASE + ["--llm_mlp_weights", "fp8", "--llm_mlp_fp8_rows", "128"]).llm_mlp_fp8_rows == 128
    with pytest.raises(SystemExit):
        get_args(BASE + ["--llm_mlp_fp8_rows", "32"])


def test_server_flag():
    from bin.server import get_parser
    p = get_parser()
    assert p.parse_args(["--llm_mlp_fp8_rows", "128"]).llm_mlp_fp8_rows == 128
    with pytest.raises(SystemExit):
        p.parse_args(["--llm_mlp_fp8_rows", "32"])


def _nargs(h, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, h)
    assert m, f"include/fo_hip.h does not declare {name}"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_declares_the_entry_and_the_table_matches():
    from fo import _lib
    h = _header()
    nargs = _nargs(h, "fo_gemm_w8_rows128")
    assert nargs == _nargs(h, "fo_gemm_w8_rows")
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "fo_gemm_w8" in v)
    assert "fo_gemm_w8_rows128" in table
    assert len(table["fo_gemm_w8_rows128"][1]) == nargs
    assert table["fo_gemm_w8_rows128"] == table["fo_gemm_w8_rows"]


def test_launch_kinds_match_the_header():
    from fo import ops
    h = _header()
    enum = re.search(r"enum\s+FoLaunchKind\s*\{(.*?)\};", h, re.S).group(1)
    kinds = [int(v) for v in re.findall(r"\bFO_L_\w+\s*=\s*(\d+)", enum)]
    n = len(kinds)
    assert kinds == list(range(n))                       # dense, in order
    total = re.search(r"\bFO_LAUNCH_KINDS\s*=\s*([0-9+ ]+)", enum).group(1)
    assert sum(int(v) for v in total.split("+")) == n   # the header's own count of them
    assert len(ops.LAUNCH_KINDS) == n
    # appended after the last existing kind
    assert int(re.search(r"FO_L_GEMM_W8_ROWS128\s*=\s*(\d+)", h).group(1)) == n - 1
    assert ops.LAUNCH_KINDS[-1] == "gemm_w8_rows128"
