"""The feature benches' tables, byte for byte: each tool's `--step report` over a synthetic work file of tests/golden/bench_reports must
print what the tool printed for it before the benches were put on tools/benchsteps.py (the README there names the commit).  No GPU, no
torch: the report step of a bench opens neither."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORTS = os.path.join(ROOT, "tests", "golden", "bench_reports")

CASES = [  # tool, work file, arguments beside the defaults, expected text
    ("reshade", "reshade.full.jsonl", [], "reshade.full.txt"),
    ("reshade", "reshade.noparent.jsonl", [], "reshade.noparent.txt"),
    ("source_table", "source_table.full.jsonl", [], "source_table.full.txt"),
    ("source_table", "source_table.noparent.jsonl", [], "source_table.noparent.txt"),
    ("relisten", "relisten.full.jsonl", [], "relisten.full.txt"),
    ("relisten", "relisten.noparent.jsonl", [], "relisten.noparent.txt"),
    ("reshade_grad", "reshade_grad.full.jsonl", [], "reshade_grad.full.txt"),
    ("reshade_grad_map", "reshade_grad_map.full.jsonl", [], "reshade_grad_map.full.txt"),
    ("reshade_grad_map", "reshade_grad_map.noparent.jsonl", [], "reshade_grad_map.noparent.txt"),
    ("window", "window.full.jsonl", [], "window.full.txt"),
    ("window", "window.noparent.jsonl", [], "window.noparent.txt"),
    ("decay", "decay.full.jsonl", ["--bins", "4096"], "decay.full.txt"),
    ("decay_params", "decay_params.full.jsonl", ["--bins", "4096"], "decay_params.full.txt"),
    ("decay_params", "decay_params.noparent.jsonl", ["--bins", "4096"], "decay_params.noparent.txt"),
    ("early_fit", "early_fit", ["--parent-lib", "parent.so"], "early_fit.full.txt"),      # early_fit.cathedral, .room, .turns
    ("early_fit", "early_fit", [], "early_fit.noparent.txt"),
]


def report(tool, work, extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool + "_bench.py"), "--step", "report", "--work", work] + extra,
                          check=True, capture_output=True).stdout


@pytest.mark.parametrize("tool,work,extra,expected", CASES, ids=[c[3][:-4] for c in CASES])
def test_report_text_is_unchanged(tool, work, extra, expected):
    with open(os.path.join(REPORTS, expected), "rb") as f:
        want = f.read()
    assert report(tool, os.path.join(REPORTS, work), extra) == want


def test_out_file_holds_the_table(tmp_path):
    out = tmp_path / "table.txt"
    printed = report("reshade", os.path.join(REPORTS, "reshade.full.jsonl"), ["--out", str(out)])
    assert out.read_bytes() == printed


def test_grad_map_out_file_keeps_its_notes(tmp_path):
    out = tmp_path / "table.txt"
    out.write_text("an older table\n---- notes\nkept\n")
    printed = report("reshade_grad_map", os.path.join(REPORTS, "reshade_grad_map.full.jsonl"), ["--out", str(out)])
    assert out.read_bytes() == printed + b"\n---- notes\nkept\n"
