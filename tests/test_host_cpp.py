"""CPU-only: the C++ host programs build, their PNG codec (arap_flow_amd/host/png_io.cpp, independent of the
reference's vendored LodePNG) decodes every PNG flavour the pipeline meets exactly as PIL does, and their list-line
grammar (arap_flow_amd/host/list_line.h) reads every line to the fields its Python twin reads."""
import os
import os.path as osp
import subprocess

import numpy as np
import pytest
from PIL import Image

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))


@pytest.fixture(scope="module")
def bins():
    from arap_flow_amd import build
    outs = build.build_host()
    return {osp.basename(o): o for o in outs}


def test_host_programs_build_and_print_usage(bins):
    for name in ("arap_deform", "warp_image"):
        assert osp.exists(bins[name])
    # argument errors are handled before any GPU call (there is no GPU here): same message + exit code 1 as the
    # reference (main.cpp:193-197, warping main.cpp:312-316)
    for name in ("arap_deform", "warp_image"):
        r = subprocess.run([bins[name], "just", "two"], capture_output=True, text=True)
        assert r.returncode == 1 and "Invalid Input!" in r.stdout and "Usage" in r.stdout


@pytest.mark.parametrize("mode", ["RGB", "RGBA", "L", "LA", "P", "1", "I;16", "L2", "L4"])
def test_png_codec_matches_pil(bins, tmp_path, mode, golden_dir):
    rng = np.random.default_rng(3)
    H, W = 37, 53                                         # odd sizes: sub-byte rows need padding
    src = str(tmp_path / "in.png")
    if mode == "RGB":
        Image.fromarray(rng.integers(0, 256, (H, W, 3)).astype(np.uint8)).save(src)
    elif mode == "RGBA":
        Image.fromarray(rng.integers(0, 256, (H, W, 4)).astype(np.uint8)).save(src)
    elif mode == "L":
        Image.fromarray(rng.integers(0, 256, (H, W)).astype(np.uint8)).save(src)
    elif mode == "LA":
        Image.fromarray(rng.integers(0, 256, (H, W, 2)).astype(np.uint8), "LA").save(src)
    elif mode == "P":
        im = Image.fromarray(rng.integers(0, 7, (H, W)).astype(np.uint8), "P")
        im.putpalette(list(rng.integers(0, 256, 21)))
        im.save(src)
    elif mode == "1":
        Image.fromarray(rng.random((H, W)) < 0.5).save(src)
    elif mode == "I;16":
        Image.fromarray((rng.integers(0, 65536, (H, W))).astype(np.uint16)).save(src)
    else:                                                  # 2- and 4-bit greyscale via PIL's bits option
        bits = int(mode[1])
        Image.fromarray(rng.integers(0, 1 << bits, (H, W)).astype(np.uint8), "P").save(src, bits=bits)
    r = subprocess.run([bins["png_tool"], src, str(tmp_path / "o.png"), str(tmp_path / "m.png")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.split() == [str(W), str(H)]
    got = np.array(Image.open(tmp_path / "o.png"))
    if mode == "I;16":
        ref = np.stack([(np.array(Image.open(src)) >> 8).astype(np.uint8)] * 3, -1)       # high byte
    else:
        ref = np.array(Image.open(src).convert("RGB"))
    assert got.shape == (H, W, 3) and np.array_equal(got, ref)
    m = Image.open(tmp_path / "m.png")
    assert m.mode == "1" and np.array_equal(np.array(m), ref[..., 0] != 0)


def test_png_codec_reads_reference_fixtures(bins, tmp_path, golden_dir):
    for f in ("cat512_iRGB.png", "cat512_iMsk.png", "cat512_wMsk.png"):
        src = osp.join(golden_dir, "cat512", f)
        r = subprocess.run([bins["png_tool"], src, str(tmp_path / "o.png"), str(tmp_path / "m.png")], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout
        assert np.array_equal(np.array(Image.open(tmp_path / "o.png")), np.array(Image.open(src).convert("RGB")))


# ---- the list line: host/list_line.h against pipeline.parse_line ------------------------------------------------------
_SIX = "a b c d e f"
_LAY = "layers R 1 m1 f1"
_M = "1,0,3,0,1,4,1,0,3.5,0,1,4.25"
_BG = "bg B r1 m1 r2 m2 F"
LINE_CORPUS = [
    _SIX, "a b c d e", "",
    _SIX + " junk x=y bwd=B.flo occ=O.png occ_bwd=OB.png", _SIX + " bwd= occ=O.png", _SIX + " bwd=X bwd=Y",
    # mid= on a solve line: accepted (the last is ignored) ...
    _SIX + " mid=4,9,14:pre", _SIX + " mid=1,2,3,4,5,6,7,8:p", _SIX + " mid=04:p", _SIX + " mid=4:p:q", _SIX + " mid=",
    # ... and refused
    _SIX + " mid=4,4:pre", _SIX + " mid=0:pre", _SIX + " mid=4,:pre", _SIX + " mid=,4:pre", _SIX + " mid=4:", _SIX + " mid=:pre",
    _SIX + " mid=1,2,3,4,5,6,7,8,9:p",
    "layers R 2 m1 f1 m2 f2 occ=O",
    _LAY + " mid=4,9:P occ=O rgb2=R2 mask2=M2 bwd=B occ_bwd=OB",                          # done = 4,9:P
    "layers R 2 m1 f1 m2 f2", "layers R 2 m1 f1 m2 occ=O", "layers R 0 occ=O", "layers R 256 occ=O", "layers R x m1 f1 occ=O",
    _LAY + " foo=O", _LAY + " occ=", _LAY + " junk", _LAY + " mid=9,4:P", "layers",
    _BG + " m=" + _M + " out=a,b,c", _BG + " m=" + _M + " out=,,c",
    _BG + " m=" + _M + " occ=O occ_out=OO bwd=Bi bwd_out=BO occ_bwd=OBi occ_bwd_out=OBO",  # done = OO
    _BG + " m=0.1,0.2,0.3,1e10,1,4,1,0,3.5,0,1,4.25 out=a,b,c",                           # %.9g of float32
    _BG + " m=" + _M + " out=,,", _BG + " m=" + _M + " out=a,b", _BG + " m=" + _M + " out=a,b,c,d",
    _BG + " m=" + _M[:-5] + " out=a,b,c", _BG + " m=" + _M + ",7 out=a,b,c", _BG + " m=" + _M[:-4] + "x out=a,b,c",
    _BG + " m=" + _M[:-4] + "1, out=a,b,c", _BG + " out=a,b,c", _BG + " m=" + _M + " occ_out=OO",
    _BG + " m=" + _M + " occ=O", _BG + " m=" + _M + " out=a,b,c foo=1", "bg B r1 m1 r2 m2 m=" + _M + " out=a,b,c",
]


def test_list_line_parser_equals_python_twin(bins):
    """every line of the corpus through line_tool in one process: a line pipeline.parse_line accepts comes back as
    exactly format_line(parse_line(line)) + " done=" + done_token, one it refuses as SKIP or BAD.  (Left out, because the
    twins disagree there: mid=+4:p and mid=1234567:p, which only Python accepts, and a repeated key on a layers line,
    whose done path differs.)"""
    from arap_flow_amd import pipeline
    assert len(_M.split(",")) == 12 and len(_M[:-5].split(",")) == 11
    r = subprocess.run([bins["line_tool"]], input="".join(c + "\n" for c in LINE_CORPUS), capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr
    got = [ln for ln in r.stdout.split("\n")[:-1] if not ln.startswith("Invalid")]
    assert len(got) == len(LINE_CORPUS)
    accepted = 0
    for line, g in zip(LINE_CORPUS, got):
        try:
            item = pipeline.parse_line(line)
        except ValueError:
            assert g in ("SKIP", "BAD"), (line, g)
            continue
        assert g == pipeline.format_line(item) + " done=" + pipeline.done_token(item), line
        accepted += 1
    assert accepted == 15                                  # 4 plain + 5 mid= solve lines, 2 layers, 4 bg: those marked accepted


def test_arap_deform_refuses_a_bad_list_before_any_gpu_call(bins, tmp_path):
    """a refused line ends a list run with exit code 1 and its message, a list without a line with nothing but the
    reference's message: all before the first GPU call, so the whole stdout is known here"""
    lst = tmp_path / "l.txt"
    bad_bg = _BG + " m=" + _M + " occ=O"
    bad_mid = _SIX + " mid=4,4:pre"
    for text, out in ((_SIX + "\n" + bad_bg + "\n" + _SIX + "\n", "Invalid bg line: " + bad_bg + "\n"),
                      (_SIX + "\n" + bad_mid + "\n", "Invalid mid= token: " + bad_mid + "\n"),
                      ("a b c d e\n\nx\n", "No file to be processed")):
        lst.write_text(text)
        r = subprocess.run([bins["arap_deform"], str(lst)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stdout == out, (text, r.stdout, r.stderr)
