"""Generated cfg text == the reference's cfg files, block by block (their parsed blocks: tests/golden/live_checks.json,
minted by tests/golden/make_golden.py; CPU only)."""
import os
import sys

import pytest

from fewshot_detection_amd import cfgs
from fewshot_detection_amd.cfg import parse_cfg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden  # noqa: E402


def _norm(blocks):
    return [{k: str(v).replace(" ", "") for k, v in b.items()} for b in blocks]


def test_generated_cfgs_equal_reference_files(tmp_path):
    dyn, rw, tiny = cfgs.write_standard_cfgs(str(tmp_path))
    gold = make_golden.live_checks()[0]["cfg_blocks"]
    for mine, ref in ((dyn, "darknet_dynamic.cfg"), (rw, "reweighting_net.cfg"), (tiny, "tiny-yolo-voc.cfg")):
        a = _norm(parse_cfg(mine))
        b = gold[ref]
        assert len(a) == len(b), ref
        for i, (x, y) in enumerate(zip(a, b)):
            assert x == y, (ref, i, x, y)


def test_cfg_parser_basics(tmp_path):
    p = tmp_path / "t.cfg"
    p.write_text("# comment\n[net]\nwidth = 32\n\n[convolutional]\nfilters=8\n[cost]\ntype=sse\n")
    blocks = parse_cfg(str(p))
    assert blocks[0] == {"type": "net", "width": "32"}
    assert blocks[1] == {"type": "convolutional", "batch_normalize": 0, "filters": "8"}
    assert blocks[2] == {"type": "cost", "_type": "sse"}
