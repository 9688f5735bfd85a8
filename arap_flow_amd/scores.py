"""Score tables off the GPU: their names, their files' text, pooling and the metrics (DESIGN.md "Flow scoring", "Track
scoring", "Frame scoring", "Map scoring").  Everything about a score that is not a list line; numpy, re and math only, so
opt.py and pipeline.py both import it.  pipeline re-exports every function here under the same name.

A score file is rows `<head words> key=int key=int ...` of unsigned 64-bit integers (format_row, parse_row); the C++
worker writes the same bytes (host/device_pass.h).  The flow and the frame table are a FixedTable; track, label and map
files have their own row structure and their own short loops over the two row functions.
"""
import math
import re
from typing import NamedTuple

import numpy as np

# the rows and the fields of each table in its order (ArapFlow_FlowScore, _TrackScore, _FrameScore, _LabelScore, _MapScore)
SCORE_ROWS = ("all", "noc", "occ", "d0-10", "d10-60", "d60-140", "s0-10", "s10-40", "s40+", "left_out")
SCORE_FIELDS = ("count", "sum", "n1", "n3", "n5", "fl", "nonfinite", "max")
FSCORE_ROWS = ("all", "noc", "occ", "d0-10", "d10-60", "d60-140", "obj", "bg", "left_out")
FSCORE_FIELDS = ("count", "sse", "sad", "max", "windows", "ssim_sum", "ssim_worst")
TSCORE_MAX_FRAMES = 64       # ARAPFLOW_TSCORE_MAX_FRAMES of include/arap_opt.h
TSCORE_CLASSES = ("all", "tracked", "reappeared")
TSCORE_X = (1, 2, 4, 8, 16)
TSCORE_FIELDS = ("count", "gt_vis", "est_vis", "agree") + tuple("within_%d" % x for x in TSCORE_X) + \
                tuple("tp_%d" % x for x in TSCORE_X) + ("sum", "max")
LSCORE_FRAME_FIELDS = ("counted", "skipped", "equal", "gt_above", "est_above")       # row 0 of a label table
# A label's row has 8 fields, the last always zero: opt.LSCORE_FIELDS is all 8, the table's width; a file leaves the zero
# out, and pipeline.LSCORE_FIELDS is the 7 it writes.  One name, two values, as before: nothing here uses the bare name.
LSCORE_TABLE_FIELDS = ("gt", "est", "inter", "gt_b", "est_b", "gt_hit", "est_hit", "zero")
LSCORE_FILE_FIELDS = LSCORE_TABLE_FIELDS[:-1]
MSCORE_MAX_THR = 8           # ARAPFLOW_MSCORE_MAX_THR of include/arap_opt.h
MSCORE_MATCH_FIELDS = ("a", "b", "a_hit", "b_hit")


def format_row(head, keys, values):
    """`<head words> key=int ...` of the values in the order of `keys`, without a newline"""
    return " ".join(list(head) + ["%s=%d" % (k, int(v)) for k, v in zip(keys, values)])


def parse_row(what, line, head, keys):
    """the inverse of format_row: the integers of `<head> key=int ...` in the order of `keys`"""
    tok = line.split(" ")
    if tok[:len(head)] != list(head) or len(tok) != len(head) + len(keys):
        raise ValueError("%s: bad row %r" % (what, line))
    out = []
    for key, cell in zip(keys, tok[len(head):]):
        k, _, v = cell.partition("=")
        if k != key or not re.match(r"[0-9]{1,20}$", v) or int(v) >= 1 << 64:
            raise ValueError("%s: bad field %r" % (what, cell))
        out.append(int(v))
    return out


class FixedTable(NamedTuple):
    """a table uint64[rows][fields] whose file has one line per row name; the last row has only its two `last` keys.
    Pooled, the fields `peaks` of every row but the last take the maximum, every other field the integer sum."""
    what: str
    rows: tuple
    fields: tuple
    last: tuple
    peaks: tuple

    def keys(self, r):
        return self.fields if r < len(self.rows) - 1 else self.last

    def array(self, table):
        return np.asarray(table, np.uint64).reshape(len(self.rows), len(self.fields))

    def format(self, table):
        return "".join(format_row([name], self.keys(r), row) + "\n" for r, (name, row) in enumerate(zip(self.rows, self.array(table))))

    def parse(self, text):
        lines = text.split("\n")
        if len(lines) != len(self.rows) + 1 or lines[-1] != "":
            raise ValueError("%s: %d lines expected" % (self.what, len(self.rows)))
        t = np.zeros((len(self.rows), len(self.fields)), np.uint64)
        for r, (name, line) in enumerate(zip(self.rows, lines)):
            cells = parse_row(self.what, line, [name], self.keys(r))
            t[r, :len(cells)] = cells
        return t

    def add(self, tables):
        out, peaks = np.zeros((len(self.rows), len(self.fields)), np.uint64), list(self.peaks)
        for t in tables:
            t = self.array(t)
            peak = np.maximum(out[:-1, peaks], t[:-1, peaks])
            out += t
            out[:-1, peaks] = peak
        return out


FLOW_TABLE = FixedTable("score file", SCORE_ROWS, SCORE_FIELDS, ("skipped", "gt_nonfinite"), (7,))
FRAME_TABLE = FixedTable("frame score file", FSCORE_ROWS, FSCORE_FIELDS, ("pixels", "windows"), (3, 6))


def format_score(table):
    """the text of a score file: one line per row of a table uint64[10][8], `<row name> count=.. sum=.. n1=.. n3=.. n5=..
    fl=.. nonfinite=.. max=..`, the last `left_out skipped=.. gt_nonfinite=..`; integers only; the C++ worker writes the
    same bytes"""
    return FLOW_TABLE.format(table)


def parse_score_file(text):
    """the inverse of format_score -> uint64[10][8]"""
    return FLOW_TABLE.parse(text)


def add_scores(tables):
    """the pooled table of several: the integer sum of every field but `max`, which is the maximum -- exactly the table
    of all their pixels together"""
    return FLOW_TABLE.add(tables)


def score_summary(table):
    """{row name: dict(count, epe, r1, r3, r5, fl)} of a table, float64: the mean end-point error in pixels and the
    outlier rates as fractions of the row's count (nan for an empty row); `left_out` is dict(skipped, gt_nonfinite)"""
    t = np.asarray(table, np.uint64).reshape(len(SCORE_ROWS), len(SCORE_FIELDS))
    res = {}
    for name, row in zip(SCORE_ROWS[:-1], t):
        count, total, n1, n3, n5, fl = (float(int(v)) for v in row[:6])
        over = lambda v: v / count if count else float("nan")
        res[name] = dict(count=int(row[0]), epe=over(total / 4096.0), r1=over(n1), r3=over(n3), r5=over(n5), fl=over(fl))
    res[SCORE_ROWS[-1]] = dict(skipped=int(t[-1, 0]), gt_nonfinite=int(t[-1, 1]))
    return res


def format_frame_score(table):
    """the text of a frame score file: one line per row of a table uint64[9][7], `<row name> count=.. sse=.. sad=.. max=..
    windows=.. ssim_sum=.. ssim_worst=..`, the last `left_out pixels=.. windows=..`; integers only; the C++ worker writes
    the same bytes"""
    return FRAME_TABLE.format(table)


def parse_frame_score_file(text):
    """the inverse of format_frame_score -> uint64[9][7]"""
    return FRAME_TABLE.parse(text)


def add_frame_scores(tables):
    """the pooled table of several: the integer sum of every field but `max` and `ssim_worst`, which take the maximum --
    exactly the table of all their frames together"""
    return FRAME_TABLE.add(tables)


def frame_score_summary(table):
    """{row name: dict(count, psnr, mae, windows, ssim, ssim_min)} of a table, float64: psnr = 10 log10(255^2 * 3 * count /
    sse) in dB (inf when sse = 0), mae = sad / (3 * count), ssim = ssim_sum / windows / 2^20 - 1, ssim_min = 1 - ssim_worst
    / 2^20; nan for a row without pixels (psnr, mae) or windows (ssim, ssim_min); `left_out` is dict(pixels, windows)"""
    t = np.asarray(table, np.uint64).reshape(len(FSCORE_ROWS), len(FSCORE_FIELDS))
    res, nan = {}, float("nan")
    for name, row in zip(FSCORE_ROWS[:-1], t):
        count, sse, sad, _, windows, ssim_sum, worst = (int(v) for v in row)
        psnr = nan if not count else float("inf") if not sse else 10.0 * math.log10(65025.0 * 3.0 * count / sse)
        res[name] = dict(count=count, psnr=psnr, mae=sad / (3.0 * count) if count else nan, windows=windows,
                         ssim=ssim_sum / windows / 1048576.0 - 1.0 if windows else nan,
                         ssim_min=1.0 - worst / 1048576.0 if windows else nan)
    res[FSCORE_ROWS[-1]] = dict(pixels=int(t[-1, 0]), windows=int(t[-1, 1]))
    return res


def format_track_score(table):
    """the text of a track score file: one line per frame and class of a table uint64[F][3][16], `<frame> <class name>
    count=.. gt_vis=.. est_vis=.. agree=.. within_1=.. .. tp_16=.. sum=.. max=..`, frame 0 first (its `all` line holds the
    number of valid points as count and of invalid ones as gt_vis); integers only; the C++ worker writes the same bytes"""
    t = np.asarray(table, np.uint64).reshape(-1, len(TSCORE_CLASSES), len(TSCORE_FIELDS))
    return "".join(format_row(["%d" % f, name], TSCORE_FIELDS, row) + "\n"
                   for f, frame in enumerate(t) for name, row in zip(TSCORE_CLASSES, frame))


def parse_track_score_file(text):
    """the inverse of format_track_score -> uint64[F][3][16]"""
    lines = text.split("\n")
    nc = len(TSCORE_CLASSES)
    if len(lines) < 2 * nc + 1 or (len(lines) - 1) % nc or lines[-1] != "" or (len(lines) - 1) // nc > TSCORE_MAX_FRAMES:
        raise ValueError("track score file: %d lines per frame, 2..%d frames expected" % (nc, TSCORE_MAX_FRAMES))
    t = np.zeros(((len(lines) - 1) // nc, nc, len(TSCORE_FIELDS)), np.uint64)
    for r, line in enumerate(lines[:-1]):
        t[r // nc, r % nc] = parse_row("track score file", line, [str(r // nc), TSCORE_CLASSES[r % nc]], TSCORE_FIELDS)
    return t


def add_track_scores(tables):
    """the pooled table of several: tables of fewer frames are padded with zeros to the longest, every field is summed but
    `max`, which is the maximum -- exactly the table of all their points together"""
    ts = [np.asarray(t, np.uint64).reshape(-1, len(TSCORE_CLASSES), len(TSCORE_FIELDS)) for t in tables]
    out = np.zeros((max(len(t) for t in ts), len(TSCORE_CLASSES), len(TSCORE_FIELDS)), np.uint64)
    for t in ts:
        peak = np.maximum(out[:len(t), :, -1], t[:, :, -1])
        out[:len(t)] += t
        out[:len(t), :, -1] = peak
    return out


def _tscore_metrics(row):
    """dict(count, gt_vis, oa, d_1 .. d_16, d_avg, j_1 .. j_16, aj, err) of one row of fields, float64; nan where a
    denominator is zero"""
    v = [float(int(x)) for x in row]
    over = lambda a, b: a / b if b else float("nan")
    count, gt_vis, est_vis, agree = v[:4]
    res = dict(count=int(row[0]), gt_vis=int(row[1]), oa=over(agree, count))
    d = [over(w, gt_vis) for w in v[4:9]]
    j = [over(tp, gt_vis + est_vis - tp) for tp in v[9:14]]
    for x, dx, jx in zip(TSCORE_X, d, j):
        res["d_%d" % x], res["j_%d" % x] = dx, jx
    res["d_avg"], res["aj"] = sum(d) / len(d), sum(j) / len(j)
    res["err"] = over(v[14] / 4096.0, gt_vis)
    return res


def track_score_summary(table):
    """the TAP-Vid numbers of a table: {class name: metrics} over the frames 1 .. F-1 together (integer sums first, the
    maximum for `max`), then "frames": [metrics of class `all` at frame f, f = 1 .. F-1] -- the drift curve -- and "valid",
    "invalid": the numbers of query points.  metrics: dict(count, gt_vis, oa = agree / count, d_x = within_x / gt_vis,
    d_avg, j_x = tp_x / (gt_vis + est_vis - tp_x), aj, err = sum / 4096 / gt_vis), the means over the five x; nan where a
    denominator is zero.  Pooled counts, not TAP-Vid's mean over videos."""
    t = np.asarray(table, np.uint64).reshape(-1, len(TSCORE_CLASSES), len(TSCORE_FIELDS))
    res = {name: _tscore_metrics(t[1:, c].sum(axis=0)) for c, name in enumerate(TSCORE_CLASSES)}
    res["frames"] = [_tscore_metrics(t[f, 0]) for f in range(1, len(t))]
    res["valid"], res["invalid"] = int(t[0, 0, 0]), int(t[0, 0, 1])
    return res


def format_label_score(table):
    """the text of a label score file, of a table uint64[L+1][8]: `frame counted=.. skipped=.. equal=.. gt_above=..
    est_above=..`, then per label `label <k> gt=.. est=.. inter=.. gt_b=.. est_b=.. gt_hit=.. est_hit=..`; integers only;
    the C++ worker writes the same bytes"""
    t = np.asarray(table, np.uint64).reshape(-1, len(LSCORE_TABLE_FIELDS))
    lines = [format_row(["frame"], LSCORE_FRAME_FIELDS, t[0])]
    lines += [format_row(["label", "%d" % k], LSCORE_FILE_FIELDS, t[k]) for k in range(1, len(t))]
    return "\n".join(lines) + "\n"


def parse_label_score_file(text):
    """the inverse of format_label_score -> uint64[L+1][8]"""
    lines = text.split("\n")
    if not 3 <= len(lines) <= 257 or lines[-1] != "":
        raise ValueError("label score file: a frame row and 1 to 255 label rows expected")
    t = np.zeros((len(lines) - 1, len(LSCORE_TABLE_FIELDS)), np.uint64)
    t[0, :len(LSCORE_FRAME_FIELDS)] = parse_row("label score file", lines[0], ["frame"], LSCORE_FRAME_FIELDS)
    for k in range(1, len(t)):
        t[k, :len(LSCORE_FILE_FIELDS)] = parse_row("label score file", lines[k], ["label", "%d" % k], LSCORE_FILE_FIELDS)
    return t


def add_label_scores(tables):
    """the pooled table of several: the integer sum field by field, a table of fewer labels padded with zero rows --
    the table of all their maps together, but that a label above a table's own L stays where that table counted it, in
    gt_above / est_above"""
    ts = [np.asarray(t, np.uint64).reshape(-1, len(LSCORE_TABLE_FIELDS)) for t in tables]
    out = np.zeros((max([len(t) for t in ts] + [2]), len(LSCORE_TABLE_FIELDS)), np.uint64)
    for t in ts:
        out[:len(t)] += t
    return out


def _pr_f(hit_est, n_est, hit_gt, n_gt):
    """(P, R, F) of a boundary match by the DAVIS toolkit's conventions for empty sets"""
    if n_est == 0 and n_gt > 0:
        P, R = 1.0, 0.0
    elif n_est > 0 and n_gt == 0:
        P, R = 0.0, 1.0
    elif n_est == 0 and n_gt == 0:
        P, R = 1.0, 1.0
    else:
        P, R = hit_est / n_est, hit_gt / n_gt
    return P, R, 2.0 * P * R / (P + R) if P + R else 0.0


def label_score_summary(table):
    """dict(labels={k: dict(J, P, R, F)}, J, F, JF, frame=dict(...)) of a table, float64: J = inter / (gt + est - inter), 1
    when the union is empty; P = est_hit / est_b and R = gt_hit / gt_b with the DAVIS toolkit's conventions (est_b = 0 <
    gt_b: 1, 0; gt_b = 0 < est_b: 0, 1; both 0: 1, 1); F = 2 P R / (P + R), 0 when P + R = 0; J, F the means over the
    labels and JF their mean"""
    t = np.asarray(table, np.uint64).reshape(-1, len(LSCORE_TABLE_FIELDS))
    labels = {}
    for k in range(1, len(t)):
        gt, est, inter, gt_b, est_b, gt_hit, est_hit = (int(v) for v in t[k, :7])
        union = gt + est - inter
        P, R, F = _pr_f(est_hit, est_b, gt_hit, gt_b)
        labels[k] = dict(J=inter / union if union else 1.0, P=P, R=R, F=F)
    J = sum(v["J"] for v in labels.values()) / len(labels)
    F = sum(v["F"] for v in labels.values()) / len(labels)
    return dict(labels=labels, J=J, F=F, JF=(J + F) / 2.0, frame={f: int(v) for f, v in zip(LSCORE_FRAME_FIELDS, t[0])})


def format_map_score(score):
    """the text of a map score file, of dict(hist uint64[2][256], thr, match uint64[m][4]): `neg` and `pos` followed by
    the 256 counts of the class, then per threshold `match thr=.. a=.. b=.. a_hit=.. b_hit=..`; integers only; the C++
    worker writes the same bytes"""
    h = np.asarray(score["hist"], np.uint64).reshape(2, 256)
    lines = [name + "".join(" %d" % int(v) for v in row) for name, row in zip(("neg", "pos"), h)]       # rows without keys
    match = np.asarray(score.get("match", ()), np.uint64).reshape(-1, 4)
    lines += [format_row(["match"], ("thr",) + MSCORE_MATCH_FIELDS, [t] + list(q)) for t, q in zip(score.get("thr", ()), match)]
    return "\n".join(lines) + "\n"


def parse_map_score_file(text):
    """the inverse of format_map_score -> dict(hist, thr, match)"""
    lines = text.split("\n")
    if not 3 <= len(lines) <= 3 + MSCORE_MAX_THR or lines[-1] != "":
        raise ValueError("map score file: two histogram rows and up to %d match rows expected" % MSCORE_MAX_THR)
    hist = np.zeros((2, 256), np.uint64)
    for c, name in enumerate(("neg", "pos")):
        tok = lines[c].split(" ")
        if tok[0] != name or len(tok) != 257 or not all(re.match(r"[0-9]{1,20}$", v) and int(v) < 1 << 64 for v in tok[1:]):
            raise ValueError("map score file: bad row %r" % lines[c][:40])
        hist[c] = [int(v) for v in tok[1:]]
    thr, match = [], np.zeros((len(lines) - 3, 4), np.uint64)
    for j, line in enumerate(lines[2:-1]):
        cells = parse_row("map score file", line, ["match"], ("thr",) + MSCORE_MATCH_FIELDS)
        if not 1 <= cells[0] <= 255:
            raise ValueError("map score file: bad threshold in %r" % line)
        thr.append(cells[0])
        match[j] = cells[1:]
    return dict(hist=hist, thr=tuple(thr), match=match)


def add_map_scores(scores):
    """the pooled score of several: the integer sums of the histograms and, threshold by threshold, of the match rows --
    exactly the score of all their maps together.  The scores have the same thresholds."""
    scores = list(scores)
    thr = tuple(scores[0]["thr"]) if scores else ()
    hist, match = np.zeros((2, 256), np.uint64), np.zeros((len(thr), 4), np.uint64)
    for s in scores:
        if tuple(s["thr"]) != thr:
            raise ValueError("add_map_scores: thresholds %r and %r" % (thr, tuple(s["thr"])))
        hist += np.asarray(s["hist"], np.uint64).reshape(2, 256)
        match += np.asarray(s["match"], np.uint64).reshape(len(thr), 4)
    return dict(hist=hist, thr=thr, match=match)


def map_score_summary(score):
    """the pixelwise precision / recall curve of a score and what follows from it, float64: with TP(t) the positives and
    FP(t) the negatives with est >= t, t = 1..255: P(t) = TP / (TP + FP), 1 when nothing is predicted, R(t) = TP / pos
    (1 without positives) -> dict(pos, neg, P, R (arrays indexed by t, entry 0 unused), f128 = F at t = 128, best_f and
    best_t (the smallest t of the best F), ap = sum_t (R(t) - R(t + 1)) P(t) with R(256) = 0, match = {thr: dict(P, R, F)}
    by the conventions of label_score_summary)"""
    h = np.asarray(score["hist"], np.uint64).reshape(2, 256)
    neg, pos = [[int(v) for v in row] for row in h]
    n_pos = sum(pos)
    P, R, F = [float("nan")] * 256, [float("nan")] * 256, [float("nan")] * 256
    tp = fp = 0
    for t in range(255, 0, -1):
        tp, fp = tp + pos[t], fp + neg[t]
        P[t] = tp / (tp + fp) if tp + fp else 1.0
        R[t] = tp / n_pos if n_pos else 1.0
        F[t] = 2.0 * P[t] * R[t] / (P[t] + R[t]) if P[t] + R[t] else 0.0
    ap = sum((R[t] - (R[t + 1] if t < 255 else 0.0)) * P[t] for t in range(1, 256))
    best_t = max(range(1, 256), key=lambda t: (F[t], -t))
    match = {}
    for t, q in zip(score.get("thr", ()), np.asarray(score.get("match", ()), np.uint64).reshape(-1, 4)):
        a, b, a_hit, b_hit = (int(v) for v in q)
        match[int(t)] = dict(zip("PRF", _pr_f(b_hit, b, a_hit, a)))
    return dict(pos=n_pos, neg=sum(neg), P=np.asarray(P), R=np.asarray(R), f128=F[128], best_f=F[best_t], best_t=best_t,
                ap=ap, match=match)
