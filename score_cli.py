"""What score_gen.py, track_score_gen.py, frame_score_gen.py and map_score_gen.py share: the options of the GPU workers,
the run of list lines on para_gen.py's workers -- with lines that wait for another line's output -- and the two files
each of them leaves in the dataset."""
import os.path as osp
import sys
import threading

HERE = osp.dirname(osp.abspath(__file__))
sys.path.insert(0, HERE)
import para_gen                             # noqa: E402
from arap_flow_amd import pipeline          # noqa: E402


def add_worker_options(parser):
    parser.add_argument("--gpu", nargs="*", type=int, default=[0], help="GPU ids, default 0")
    parser.add_argument("--narap", type=int, default=64, help="lines one GPU holds at a time")
    parser.add_argument("--arap_bin", default=para_gen.CPP_BIN if osp.exists(para_gen.CPP_BIN) else
                        "%s %s" % (sys.executable, osp.join(HERE, "arap_deform.py")), help="this repository's arap_deform")
    parser.add_argument("--worker", choices=["auto", "serve", "batch"], default="auto", help="as para_gen.py's --worker")


def check_driver(parser, flags, lines):
    """`lines`: the script's own lines in words, "a `score` line" """
    if not para_gen.own_arap_bin(flags.arap_bin):
        parser.error("--arap_bin: %s needs this repository's driver" % lines)


def run_lines(flags, now, after=None):
    """every line (a pipeline *Line) of `now` on the workers of flags.gpu, and every line of after[t] once the line with
    pipeline.done_token t is done: a chain line's track file -> the tscore line that reads it, an interp line's prefix ->
    the fscore lines of its frames.  Returns when every line was reported done, each exactly once; starts no worker
    without a line."""
    after = after or {}
    expected = [pipeline.done_token(it) for it in list(now) + [it for owed in after.values() for it in owed]]
    done, lock = [], threading.Lock()
    workers = None

    def on_done(path):
        with lock:
            done.append(path)
        for it in after.get(path, ()):
            workers.put_owed(pipeline.format_line(it))
    if expected:
        workers = para_gen.GpuWorkers(flags.arap_bin, flags.gpu, flags.narap, para_gen.serves(flags), on_done)
        for _ in expected[len(now):]:
            workers.owe()
        for it in now:
            workers.put(pipeline.format_line(it))
        workers.close()
        workers.join()
    assert sorted(done) == sorted(expected), "a line was not reported done"


def write_results(data, name, text, missing):
    """OUT/<name>.txt, the pooled score as its file's text, and OUT/<name>_missing.list, a ground-truth file per line"""
    with open(osp.join(data, name + ".txt"), "w") as f:
        f.write(text)
    with open(osp.join(data, name + "_missing.list"), "w") as f:
        f.write("".join(m + "\n" for m in missing))
