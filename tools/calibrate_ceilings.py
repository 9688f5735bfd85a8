"""GPU box: measured ceilings for the utilisation figures of bench.py's roofline.

    python tools/calibrate_ceilings.py [--round r03]
    python tools/calibrate_ceilings.py --cells [--round r11] [--lines FILE] [--out PATH]

Builds tools/microbench/issue_peak.hip, runs it plain (cycles per instruction from in-kernel stamps) and under
rocprofv3 --pmc with the SAME counter groups tools/collect_profile.py uses, and writes
gpurun_out/profiles/<round>_ceilings.json:
  valu_active_ceiling   the largest SQ_ACTIVE_INST_VALU x 4 / (1024 SIMDs x kernel cycles) any VALU kernel reaches
  cycles per v_fma_f32 / v_pk_fma_f32 / phase-A mix, at one and two wavefronts per SIMD
  lds bytes per clock per CU for ds_read_b64 / ds_read_b32, and the counters' reading of a saturated LDS pipe

--cells runs only the four phase-A read forms of the microbench (mixlds_now / _cell / _c128 / _celladd: the same 20 words per
vertex in 12, 6, 8 and 6 LDS instructions), three rounds alternating, and writes profiles/<round>_ceilings_lds.json (or --out PATH):
cycles per vertex and wavefront of every run, their spread, and what one LDS instruction costs in that mix.  (--lines FILE
condenses the JSON lines of runs already made instead of running.)  The record of the first mode is not touched.
"""
import argparse
import collections
import csv
import glob
import json
import os
import shutil
import subprocess
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = {"sq_valu": ["SQ_ACTIVE_INST_VALU", "SQ_INSTS_VALU", "SQ_BUSY_CYCLES", "SQ_WAVE_CYCLES"],
          "sq_wait": ["SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "SQ_THREAD_CYCLES_VALU"],
          "sq_lds": ["SQ_ACTIVE_INST_LDS", "SQ_INSTS_LDS", "SQ_LDS_IDX_ACTIVE", "SQ_LDS_BANK_CONFLICT"],
          "sq_lds2": ["SQ_WAIT_INST_LDS", "SQ_LDS_ADDR_CONFLICT", "SQ_INST_LEVEL_LDS", "SQ_BUSY_CU_CYCLES"],
          "grbm": ["GRBM_GUI_ACTIVE"]}
SHORT = {"0": "fma", "1": "pkfma", "2": "mix", "3": "lds64", "4": "lds32", "5": "mixlds"}


CELL_KERNELS = ("mixlds_now", "mixlds_cell", "mixlds_c128", "mixlds_celladd")


def cells_record(lines):
    """the phase-A read forms: cycles per vertex and wavefront of every run, spread, cost of one LDS instruction"""
    runs = collections.OrderedDict()
    insts = {}
    for p in lines:
        if p["kernel"] in CELL_KERNELS:
            runs.setdefault("%s.%d_per_simd" % (p["kernel"], p["waves_per_simd"]), []).append(p["cycles_per_iter_per_wave"])
            insts[p["kernel"]] = p["lds_insts_per_iter"]
    rec = {"made_by": "tools/calibrate_ceilings.py --cells", "unix_time": int(time.time()),
           "what": "tools/microbench/issue_peak.hip cells, rounds alternating on one box: shader cycles per vertex and wavefront "
                   "(loop cycles of wave 0, median over the workgroups, / iterations / wavefronts per SIMD); every kernel issues the "
                   "same 50 VALU instructions (celladd: 52) and fetches the same 20 words",
           "lds_insts_per_vertex": insts, "cycles_per_vertex": {}, "plain": lines}
    for k, v in runs.items():
        rec["cycles_per_vertex"][k] = {"runs": v, "mean": sum(v) / len(v), "max_minus_min": max(v) - min(v)}
    m = {k: e["mean"] for k, e in rec["cycles_per_vertex"].items()}
    if all("%s.2_per_simd" % k in m for k in CELL_KERNELS):
        now, cell, c128, add = (m["%s.2_per_simd" % k] for k in CELL_KERNELS)
        r = rec["cycles_per_vertex"]
        rec["at_two_wavefronts_per_simd"] = {
            "every_cell_run_below_every_now_run": max(r["mixlds_cell.2_per_simd"]["runs"]) < min(r["mixlds_now.2_per_simd"]["runs"]),
            "cycles_per_lds_inst_b64_pairs_to_b128": (now - c128) / (insts["mixlds_now"] - insts["mixlds_c128"]),
            "cycles_per_lds_inst_b32_pairs_to_read2": (c128 - cell) / (insts["mixlds_c128"] - insts["mixlds_cell"]),
            "cycles_per_address_v_add_u32": (add - cell) / 2.0}
    return rec


def cells(a):
    if a.lines:
        lines = [json.loads(ln) for ln in open(a.lines) if ln.startswith("{")]
    else:
        exe = "/tmp/issue_peak"
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-o", exe,
                               os.path.join(ROOT, "tools", "microbench", "issue_peak.hip")])
        lines = []
        for _ in range(3):
            out = subprocess.run([exe, "cells"], capture_output=True, text=True, check=True).stdout
            lines += [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
    rec = cells_record(lines)
    path = a.out or os.path.join(ROOT, "profiles", "%s_ceilings_lds.json" % a.round)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write(json.dumps(rec, indent=1) + "\n")
    print("wrote", path)
    print(json.dumps({k: v for k, v in rec.items() if k != "plain"}, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--round", default="r03")
    ap.add_argument("--cells", action="store_true", help="only the phase-A read forms: <round>_ceilings_lds.json")
    ap.add_argument("--lines", default=None, help="with --cells: condense these recorded JSON lines instead of running")
    ap.add_argument("--out", default=None, help="with --cells: where the record goes (default profiles/<round>_ceilings_lds.json)")
    a = ap.parse_args()
    if a.cells:
        return cells(a)
    os.chdir("/tmp")
    os.environ["TMPDIR"] = "/tmp"
    exe = "/tmp/issue_peak"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-o", exe,
                           os.path.join(ROOT, "tools", "microbench", "issue_peak.hip")])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    plain = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
    rec = {"made_by": "tools/calibrate_ceilings.py", "unix_time": int(time.time()), "plain": plain, "pmc": {}}
    for tag, ctrs in GROUPS.items():
        d = "/tmp/cal_%s" % tag
        shutil.rmtree(d, ignore_errors=True)
        r = subprocess.run(["rocprofv3", "--pmc"] + ctrs + ["--output-format", "csv", "-d", d, "--", exe],
                           capture_output=True, text=True)
        files = glob.glob(d + "/**/*counter_collection.csv", recursive=True)
        if r.returncode != 0 or not files:
            rec["pmc"][tag] = {"error": (r.stderr or r.stdout)[-300:]}
            continue
        # dispatches come in the order the program launches them: per kernel (warm-up, timed) x (2 per CU, 1 per CU)
        per = collections.OrderedDict()
        for row in csv.DictReader(open(files[0])):
            key = (row["Kernel_Name"], int(row["Dispatch_Id"]))
            cs = per.setdefault(key, {})
            cs[row["Counter_Name"]] = cs.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
        by_kernel = collections.OrderedDict()
        for (name, disp), cs in sorted(per.items(), key=lambda kv: kv[0][1]):
            by_kernel.setdefault(name, []).append(cs)
        for name, lst in by_kernel.items():
            idx = name.split("<")[-1].split(">")[0].replace("(int)", "").strip()
            short = SHORT.get(idx, name)
            timed = {"2_per_cu": lst[1] if len(lst) > 1 else None, "1_per_cu": lst[3] if len(lst) > 3 else None}
            rec["pmc"].setdefault(short, {})
            for k, cs in timed.items():
                if cs:
                    rec["pmc"][short].setdefault(k, {}).update(cs)
        shutil.rmtree(d, ignore_errors=True)
    # ---- derived ceilings -------------------------------------------------------------------------------------------
    der = {}
    ms = {(p["kernel"], p["waves_per_simd"]): p for p in plain}
    for short, occ in rec["pmc"].items():
        if short in GROUPS or not isinstance(occ, dict):
            continue
        for k, cs in occ.items():
            w = 2 if k.startswith("2") else 1
            p = ms.get((short, w))
            if not p or not isinstance(cs, dict):
                continue
            cycles = p["ms"] * 1e-3 * p["clock_MHz"] * 1e6          # kernel duration in shader clocks (measured clock)
            e = {"kernel_cycles": cycles}
            if "SQ_ACTIVE_INST_VALU" in cs:
                e["valu_active_x4_per_simd_cycle"] = cs["SQ_ACTIVE_INST_VALU"] * 4.0 / (1024.0 * cycles)
                e["valu_insts_per_simd_cycle"] = cs.get("SQ_INSTS_VALU", 0.0) / (1024.0 * cycles)
            if "SQ_ACTIVE_INST_LDS" in cs:
                e["lds_active_x4_per_cu_cycle"] = cs["SQ_ACTIVE_INST_LDS"] * 4.0 / (256.0 * cycles)
                e["lds_idx_active_per_cu_cycle"] = cs.get("SQ_LDS_IDX_ACTIVE", 0.0) / (256.0 * cycles)
                e["lds_insts_per_cu_cycle"] = cs.get("SQ_INSTS_LDS", 0.0) / (256.0 * cycles)
            der.setdefault(short, {})[k] = e
    rec["derived"] = der
    vals = [e["valu_active_x4_per_simd_cycle"] for occ in der.values() for e in occ.values()
            if "valu_active_x4_per_simd_cycle" in e]
    rec["valu_active_ceiling"] = max(vals) if vals else None
    lvals = [e["lds_idx_active_per_cu_cycle"] for k in ("lds64", "lds32") for e in der.get(k, {}).values()
             if "lds_idx_active_per_cu_cycle" in e]
    rec["lds_idx_active_ceiling"] = max(lvals) if lvals else None
    prof = os.path.join(ROOT, "gpurun_out", "profiles")
    os.makedirs(prof, exist_ok=True)
    path = os.path.join(prof, "%s_ceilings.json" % a.round)
    open(path, "w").write(json.dumps(rec, indent=1) + "\n")
    print("wrote", path)
    for p in plain:
        print(p)
    print(json.dumps(der, indent=1)[:6000])
    print("valu_active_ceiling", rec["valu_active_ceiling"], "lds_idx_active_ceiling", rec["lds_idx_active_ceiling"])


if __name__ == "__main__":
    main()
