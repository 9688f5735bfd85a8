"""The list-line grammar as a table (arap_flow_amd/lines.py) and the list runner (run_lines.run_list), without a GPU.

tests/golden/host/list_lines.json is what the code BEFORE the table made of every list line the host tests hold (their
corpora, 478 lines) and of a few lines for the deliberately loose behaviours: per line either `refused`, or the parsed
item as plain JSON, format_line of it and done_token of it.  The grammar must still give exactly that."""
import json
import os.path as osp
import subprocess
import sys

import pytest

from arap_flow_amd import lines, run_lines

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
WORDS = {lines.LAYERS_WORD, lines.BG_WORD, lines.TEX_WORD, lines.TRK_WORD, lines.BLUR_WORD, lines.LIGHT_WORD, lines.SEG_WORD,
         lines.SCORE_WORD, lines.TSCORE_WORD, lines.CHAIN_WORD, lines.FSCORE_WORD, lines.INTERP_WORD, lines.LSCORE_WORD,
         lines.MSCORE_WORD}


def _plain(v):
    """an item as JSON holds it: NamedTuples and dicts as objects, tuples and lists as arrays"""
    if hasattr(v, "_asdict"):
        return {k: _plain(q) for k, q in v._asdict().items()}
    if isinstance(v, dict):
        return {k: _plain(q) for k, q in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(q) for q in v]
    return v


def _word(text):
    """the form a line belongs to: its first word if FORMS knows it, else None, the solve line"""
    tok = text.split()
    return tok[0] if tok and tok[0] in WORDS else None


@pytest.fixture(scope="module")
def recorded():
    with open(osp.join(ROOT, "tests", "golden", "host", "list_lines.json")) as f:
        return json.load(f)


def test_the_table_has_the_fifteen_forms():
    assert len(WORDS) == 14 and set(lines.FORMS) == WORDS | {None}
    assert all(f.word == w for w, f in lines.FORMS.items())
    assert len(lines.FORM_OF) == 15 and lines.FORMS[None].type is lines.SolveLine      # one type per form
    assert set(run_lines.RUN) == set(lines.FORM_OF) - {lines.SolveLine}                # every other form has its executor


def test_every_recorded_line_reads_writes_and_reports_as_before(recorded):
    assert len(recorded) >= 478 and len({r["line"] for r in recorded}) == len(recorded)
    accepted, refused = set(), set()
    for rec in recorded:
        text = rec["line"]
        if rec.get("refused"):
            refused.add(_word(text))
            with pytest.raises(ValueError):
                lines.parse_line(text)
            continue
        accepted.add(_word(text))
        item = lines.parse_line(text)
        assert type(item) is lines.FORMS[_word(text)].type, text
        # (as JSON text too: it tells -0.0 from 0.0 and an int from a float, which == does not)
        assert _plain(item) == rec["item"] and json.dumps(_plain(item), sort_keys=True) == json.dumps(rec["item"], sort_keys=True), text
        assert list(_plain(item)) == list(rec["item"]), text                           # the fields in their order
        if type(item) is lines.LayersLine:
            assert item._asdict() == dict(rgb=rec["item"]["rgb"], layers=[tuple(q) for q in rec["item"]["layers"]], out=rec["item"]["out"])
        assert lines.format_line(item) == rec["text"], text
        assert lines.done_token(item) == rec["done"], text
        assert lines.parse_line(lines.format_line(item)) == item, text
        assert lines.parse_line(text.split()) == item, text                            # tokens or text
    assert accepted == refused == WORDS | {None}


def test_the_loose_forms_stay_loose():
    """what the strict tail of the other forms refuses and these three accept"""
    lay = lines.parse_line("layers R 1 m f occ=O1 rgb2=B occ=O2")                      # a repeated key: first place, last value
    assert list(lay.out.items()) == [("occ", "O2"), ("rgb2", "B")] and lines.done_token(lay) == "O2"
    solve = lines.parse_line("a b c d e f junk bwd= x=y occ=O.png =v fold")            # unknown and empty tokens are dropped
    assert solve.extra == dict(occ="O.png") and lines.format_line(solve) == "a b c d e f occ=O.png"
    bg = lines.parse_line("bg B r1 m1 r2 m2 f m=1,0,0,0,1,0,1,0,0,0,1,0 out=,,c")     # empty places in out=
    assert bg.out == ("", "", "c") and lines.done_token(bg) == "c"
    for strict in ("tex R 1 m f t=0,7,1,0,0,0,1,0,0,0,1,2,3,4,5,6,7,8,9 rgb1=A rgb1=B", "score g e out=T junk", "seg 1 m f s=1,2 idx1="):
        with pytest.raises(ValueError):
            lines.parse_line(strict)


def test_lines_imports_neither_images_nor_the_library():
    code = ("import sys; import arap_flow_amd.lines; "
            "bad = [m for m in ('PIL', 'arap_flow_amd.opt', 'arap_flow_amd.flo', 'arap_flow_amd.run_lines', 'arap_flow_amd.pipeline') "
            "if m in sys.modules]; print(bad); sys.exit(1 if bad else 0)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_run_list_groups_the_solves_and_runs_every_other_line_in_its_place(monkeypatch, capsys):
    six = "r%d.png m%d.png c%d.txt f%d.flo w%d.png wm%d.png"
    items = [lines.parse_line(t) for t in (six % ((0,) * 6), six % ((1,) * 6), "score g.flo e.flo out=T.txt", six % ((2,) * 6),
                                           "layers r.png 1 m.png f.flo occ=o.png", "trk P.trk 1 1 m f out=O.trk")]
    calls = []
    monkeypatch.setattr(run_lines, "deform_list", lambda state, batch, *schedule: calls.append(("solve", state, list(batch), schedule)))
    for kind in list(run_lines.RUN):
        monkeypatch.setitem(run_lines.RUN, kind, lambda state, item, kind=kind: calls.append((kind, state, item)))
    run_lines.run_list("STATE", items, 19, 8, 400)
    assert calls == [("solve", "STATE", items[:2], (19, 8, 400)), (lines.ScoreLine, "STATE", items[2]),
                     ("solve", "STATE", items[3:4], (19, 8, 400)), (lines.LayersLine, "STATE", items[4]),
                     (lines.TrkLine, "STATE", items[5])]
    assert capsys.readouterr().out == "Saved\n" * 3                                    # one per line that is no solve
