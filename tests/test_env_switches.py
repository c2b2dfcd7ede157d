"""The environment variables the library reads are the 13 written out here, and DESIGN.md §5 documents each of them: what
it selects, who sets it and when it is read.  A switch added to the sources fails this test until it is listed here and in
that table; a switch nothing sets does not belong in the sources (a path that only a user-set option could choose is not
kept)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEPT = {
    "GIGL_LINEAR_EXACT", "GIGL_GEMM_SPLIT", "GIGL_PLAN_HS_LAYERS", "GIGL_F2_ALL_WR", "GIGL_PLAN_SELF_COPY",
    "GIGL_PLAN_NO_FUSE2", "GIGL_TRAIN_PLAN_EAGER", "GIGL_LP_FORK", "GIGL_SAMPLER_PROXY_BITS", "GIGL_DIST_OVERLAP",
    "GIGL_HGT_NO_PACK", "GIGL_UNION_LG2", "GIGL_LG3_MIN_WGS",
}


def _switches_in_sources():
    names = set()
    csrc = os.path.join(ROOT, "gigl_amd", "csrc")
    files = glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))
    assert len(files) > 10, "the library's sources were not found"
    for path in files:
        with open(path, encoding="utf-8") as f:
            names.update(re.findall(r'getenv\(\s*"(GIGL_[A-Z0-9_]*)"\s*\)', f.read()))
    return names


def _table_rows():
    """name -> cells of its row in the table under '### Environment switches' of DESIGN.md"""
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as f:
        text = f.read()
    head = "### Environment switches"
    assert head in text, "DESIGN.md has no 'Environment switches' subsection"
    section = re.split(r"^#{2,3} ", text.split(head, 1)[1], maxsplit=1, flags=re.M)[0]
    rows = {}
    for line in section.splitlines():
        m = re.match(r"^\| `(GIGL_[A-Z0-9_]*)` \|", line)
        if m:
            rows[m.group(1)] = [c.strip() for c in re.split(r"(?<!\\)\|", line.strip().strip("|"))]
    return rows


def test_sources_read_exactly_the_kept_switches():
    found = _switches_in_sources()
    assert found == KEPT, {"not listed": sorted(found - KEPT), "listed but not read": sorted(KEPT - found)}


def test_every_kept_switch_is_in_the_design_table():
    rows = _table_rows()
    assert set(rows) == KEPT, {"not in DESIGN.md": sorted(KEPT - set(rows)), "only in DESIGN.md": sorted(set(rows) - KEPT)}
    for name, cells in rows.items():
        assert len(cells) == 4 and all(cells), (name, "needs: name | selects | set by | read")
        assert "once per process" in cells[3] or "at each plan creation" in cells[3], (name, cells[3])
