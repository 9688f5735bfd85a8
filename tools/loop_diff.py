"""The PCG loop of the resident kernel as the compiler emitted it (CPU only: hipcc -S cross-compiles).

    python tools/loop_diff.py asm OUT.s            device assembly of arap_flow_amd/csrc/arapopt.hip as it is now
    python tools/loop_diff.py stats A.s [NS] [SUMS]      instruction mix of the main loop of k_pcg_resident<false, NS, SUMS>
                                                         (default 7 slots; SUMS: flat (default) or any)
    python tools/loop_diff.py diff A.s B.s [NS] [SA] [SB]  the two loops side by side with register NAMES normalised (SA / SB:
                                                         flavour taken from A / B; a file of a build from before the
                                                         flavours has one kernel per NS, which is taken whatever SA says)
    python tools/loop_diff.py pairs A.s [NS] [SUMS]      duplicated weight pairs of that loop: loop-invariant first operands of
                                                         v_pk_fma_f32 whose high half is a copy of the low half made in
                                                         front of the loop (one VGPR each that an op_sel_hi broadcast
                                                         would not need), with the kernel's VGPR count and scratch size;
                                                         without NS: the table of 7, 8, 9 slots x flat, any
    python tools/loop_diff.py copies A.s [NS] [SUMS]     the plain register copies (v_mov_b32, DPP forms not counted) of that loop
                                                         per basic block, the blocks sorted into main / tail (closing
                                                         barrier to loop header) / exit / spin
    python tools/loop_diff.py same A.s B.s        every function and kernel descriptor of A against B's of the same name,
                                                   whatever their order in the files; exit status 1 on any difference

Why: the loop runs at 253 of 256 VGPRs and ~100 SGPRs, and any change elsewhere in the kernel can change its register
allocation and instruction order.  Round 3: a build whose loop differed from its predecessor's by ONE s_waitcnt (the second
of two LDS reads of the block sum issued after the first had returned) was 2 % slower.  Diffing the normalised loops of a
build before and after a change shows such things without a GPU."""
import collections
import difflib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit_asm(out):
    from arap_flow_amd import build as b
    flags = [f for f in b.FLAGS if f not in ("-shared",)]
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", "-o", out, b.SRC]
    subprocess.check_call(cmd)


SUMS = {"any": 0, "flat": 1}           # arap_resident.h: RES_SUMS_*


def kernel_lines(path, ns, sums="flat"):
    names = ["_ZN4arap14k_pcg_residentILb0ELi%dELi%dEEEvNS_7PlanDevENS_6ResDevEi:" % (ns, SUMS[sums]),
             "_ZN4arap14k_pcg_residentILb0ELi%dEEEvNS_7PlanDevENS_6ResDevEi:" % ns]       # (builds before the flavours)
    lines = open(path).read().split("\n")
    start = next(i for n in names for i, l in enumerate(lines) if l.startswith(n))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def main_loop(fn):
    """the outermost loop that comes last in the function (the PCG loop), header to the branch back to its latch"""
    hdr = [i for i, l in enumerate(fn) if re.search(r"=>This Loop Header: Depth=1", l)][-1]
    latch = [fn[i].split(":")[0] for i in range(max(0, hdr - 12), hdr + 1) if re.match(r"^\.LBB\d+_\d+:", fn[i])]
    end = -1
    for c in latch:
        for i, l in enumerate(fn):
            if i > hdr and re.search(r"s_c?branch\w*\s+" + re.escape(c) + r"\b", l):
                end = max(end, i)
    return fn[hdr:end + 1]


def normalise(l):
    l = re.sub(r";.*", "", l)
    l = re.sub(r"\.LBB\d+_\d+", "L", l)
    l = re.sub(r"v\[\d+:\d+\]", "V2", l)
    l = re.sub(r"\bv\d+\b", "V", l)
    l = re.sub(r"s\[\d+:\d+\]", "S2", l)
    l = re.sub(r"\bs\d+\b", "S", l)
    return l.rstrip()


def stats(body):
    ins = [l.strip().split()[0] for l in body if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    c = collections.Counter(ins)
    fam = lambda p: sum(v for k, v in c.items() if k.startswith(p))
    return {"instructions": len(ins), "valu": fam("v_"), "salu": fam("s_"), "lds": fam("ds_"), "global": fam("global_"),
            "scratch": fam("scratch_"), "s_load": fam("s_load"), "v_readlane (SGPR reloads)": c.get("v_readlane_b32", 0),
            "v_writelane": c.get("v_writelane_b32", 0), "s_nop": c.get("s_nop", 0), "s_waitcnt": c.get("s_waitcnt", 0)}


def written(l):
    """registers an instruction line writes (its first operand): {n} or {lo .. hi}"""
    m = re.match(r"\s+(v_\w+|ds_read\w*|global_load\w*|buffer_load\w*)\s+v(?:\[(\d+):(\d+)\]|(\d+))", l)
    if not m or m.group(1).startswith(("v_cmp", "v_readlane", "v_readfirstlane")):
        return set()
    return set(range(int(m.group(2)), int(m.group(3)) + 1)) if m.group(2) else {int(m.group(4))}


def pairs(fn):
    """duplicated weight pairs of the main loop: v[n:n+1] is the first operand of a v_pk_fma_f32 in the loop, neither half
    is written in the loop, and the last write of v(n+1) in front of the loop is `v_mov_b32 v(n+1), vn`"""
    loop = main_loop(fn)
    hdr = next(i for i in range(len(fn)) if fn[i] is loop[0])
    live = set()
    for l in loop:
        live |= written(l)
    src0 = set()
    for l in loop:
        m = re.match(r"\s+v_pk_fma_f32\s+v\[\d+:\d+\],\s*v\[(\d+):(\d+)\]", l)
        if m and int(m.group(1)) not in live and int(m.group(2)) not in live:
            src0.add(int(m.group(1)))
    last = {}
    for l in fn[:hdr]:
        for r in written(l):
            last[r] = l
    n = 0
    for lo in sorted(src0):
        m = re.match(r"\s+v_mov_b32(?:_e32)?\s+v(\d+),\s*v(\d+)\s*$", re.sub(r";.*", "", last.get(lo + 1, "")).rstrip())
        n += bool(m and int(m.group(1)) == lo + 1 and int(m.group(2)) == lo)
    return n


def blocks(loop):
    """[(label, [instruction lines])] of a loop, split at its .LBB labels; the first block is the loop header's"""
    out = []
    for l in loop:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m or not out:
            out.append((m.group(1) if m else "<header>", []))
        if l.startswith("\t") and not l.strip().startswith((".", ";")):
            out[-1][1].append(re.sub(r"\s*;.*", "", l.strip()))
    return out


def copies(fn):
    """plain register copies (v_mov_b32 without DPP) of the main loop per basic block: [(label, kind, instructions,
    copies, the copy lines)].  Kinds: "spin" -- an inner loop (a repeated look at granules: not run in steady state);
    "exit" -- a block BEHIND the update phase's closing s_barrier (the last of the loop) that is entered by a branch from
    in front of that barrier: the landing block of `!alive` or `l + 1 == L`, which the compiler lays out next to the
    latch and which runs once per launch; "tail" -- any other block from that barrier on, the stretch between the closing
    barrier and the loop header that every iteration runs; "main" -- the rest (blocks under an exec mask or behind a
    uniform branch included: whether wave 0 alone runs them is not decided here)."""
    bl = blocks(main_loop(fn))
    closing = max(k for k, (_, ins) in enumerate(bl) if any(i.startswith("s_barrier") for i in ins))
    early = {i.split()[-1] for _, ins in bl[:closing] for i in ins if re.match(r"s_c?branch", i)}
    inner = {re.match(r"^(\.LBB\d+_\d+):", l).group(1) for l in main_loop(fn)
             if re.match(r"^\.LBB\d+_\d+:", l) and ("Depth=2" in l or "Parent Loop" in l)}
    rows = []
    for k, (name, ins) in enumerate(bl):
        mv = [i for i in ins if re.match(r"v_mov_b32(_e32|_e64)?\s", i)]
        if k == closing:                                   # only what stands behind the barrier itself is the tail's
            at = max(n for n, i in enumerate(ins) if i.startswith("s_barrier"))
            tail_mv = [i for i in ins[at:] if re.match(r"v_mov_b32(_e32|_e64)?\s", i)]
            rows.append((name, "main", len(ins), len(mv) - len(tail_mv), [i for i in mv if i not in tail_mv]))
            rows.append((name + " (behind s_barrier)", "tail", len(ins) - at - 1, len(tail_mv), tail_mv))
            continue
        kind = "spin" if name in inner else "main" if k < closing else "exit" if name in early else "tail"
        rows.append((name, kind, len(ins), len(mv), mv))
    return rows


def resources(path, ns, sums):
    """(VGPRs, scratch bytes) of the kernel, from the comment block behind its code"""
    lines = open(path).read().split("\n")
    fn = kernel_lines(path, ns, sums)
    i = next(k for k in range(len(lines)) if lines[k] == fn[0])
    tail = "\n".join(lines[i + len(fn):i + len(fn) + 400])
    return int(re.search(r"; NumVgprs: (\d+)", tail).group(1)), int(re.search(r"; ScratchSize: (\d+)", tail).group(1))


def functions(path):
    """{name: text} of every function of a device assembly file, from its "Begin function" line to the next one's, kernel
    descriptor, resource symbols and "Kernel info" included, plus "<metadata NAME>" per kernel entry of the trailing
    amdhsa.kernels list ("<head>" / "<tail>": what stands before the first and behind the last).  Labels carry the function's ordinal in the file (.LBB12_3, .Lfunc_end12): dropped, so that a
    function compares equal wherever it stands.  Lines with the per-compilation __hip_cuid_ symbol are ignored."""
    lines = [l for l in open(path).read().split("\n") if "__hip_cuid_" not in l]
    meta = next((i for i, l in enumerate(lines) if l.strip() == ".amdgpu_metadata"), len(lines))
    out, name, body = {}, "<head>", []
    for l in lines[:meta]:
        m = re.search(r"; -- Begin function (\S+)", l)
        if not m and l.split()[:1] == [".p2alignl"]:                           # padding behind the last function
            m = re.match("(<tail>)", "<tail>")
        if m:
            k = len(body)
            while k and body[k - 1].split()[:1] in ([".text"], [".section"]):   # the new function's own section line
                k -= 1
            out[name] = "\n".join(body[:k])
            name, body = m.group(1), body[k:]
        body.append(re.sub(r"(\.LBB|\bBB|\.Lfunc_end|\.Lfunc_begin)\d+", r"\1", l))
    out[name] = "\n".join(body)
    entry = []
    for l in lines[meta:]:
        if l.startswith(("  - .", "amdhsa.target")) and entry:                 # next entry / end of the list
            n = next((e.split()[-1] for e in entry if e.strip().startswith(".name:")), "?")
            out["<metadata %s>" % n] = "\n".join(entry)
            entry = []
        if entry or l.startswith("  - ."):
            entry.append(l)
    return out


def same(a, b):
    fa, fb = functions(a), functions(b)
    bad = 0
    for n in sorted(set(fa) | set(fb)):
        if n not in fa or n not in fb:
            print("only in %s: %s" % (b if n in fb else a, n))
            bad += 1
        elif fa[n] != fb[n]:
            d = list(difflib.unified_diff(fa[n].split("\n"), fb[n].split("\n"), a, b, n=1, lineterm=""))
            print("differs: %s (%d diff lines)" % (n, len(d)))
            print("\n".join(d[:40]))
            bad += 1
    kernels = sum(1 for n in fa if n.startswith("<metadata"))
    print("%d functions and %d kernel metadata entries compared, %d differ" % (len(fa) - kernels, kernels, bad))
    return 1 if bad else 0


def main():
    a = sys.argv[1:]
    if len(a) >= 2 and a[0] == "asm":
        emit_asm(a[1])
    elif len(a) >= 2 and a[0] == "stats":
        print(stats(main_loop(kernel_lines(a[1], int(a[2]) if len(a) > 2 else 7, a[3] if len(a) > 3 else "flat"))))
    elif len(a) >= 3 and a[0] == "diff":
        ns = int(a[3]) if len(a) > 3 else 7
        sa = a[4] if len(a) > 4 else "flat"
        la, lb = main_loop(kernel_lines(a[1], ns, sa)), main_loop(kernel_lines(a[2], ns, a[5] if len(a) > 5 else sa))
        print(a[1], stats(la))
        print(a[2], stats(lb))
        na = [normalise(l) for l in la if normalise(l).strip()]
        nb = [normalise(l) for l in lb if normalise(l).strip()]
        n = 0
        for l in difflib.unified_diff(na, nb, a[1], a[2], n=2, lineterm=""):
            print(l)
            n += 1
        print("(%d diff lines)" % n)
    elif len(a) >= 2 and a[0] == "pairs":
        for ns, sums in ([(int(a[2]), a[3] if len(a) > 3 else "flat")] if len(a) > 2 else
                         [(n, f) for n in (7, 8, 9) for f in ("flat", "any")]):
            st = stats(main_loop(kernel_lines(a[1], ns, sums)))
            print("%d slots, %-4s: %3d VGPRs, scratch %d, %2d duplicated weight pairs; loop: %d instructions, %d VALU, %d LDS, %d v_readlane" % (
                (ns, sums) + resources(a[1], ns, sums) + (pairs(kernel_lines(a[1], ns, sums)), st["instructions"], st["valu"],
                                                          st["lds"], st["v_readlane (SGPR reloads)"])))
    elif len(a) >= 2 and a[0] == "copies":
        rows = copies(kernel_lines(a[1], int(a[2]) if len(a) > 2 else 7, a[3] if len(a) > 3 else "flat"))
        for name, kind, n, c, mv in rows:
            print("%-4s %-36s %4d instructions, %2d v_mov_b32%s" % (kind, name, n, c, (": " + "; ".join(mv)) if mv else ""))
        tot = lambda k: sum(r[3] for r in rows if r[1] == k)
        print("v_mov_b32: %d main, %d tail (closing barrier to loop header), %d exit, %d spin" % (
            tot("main"), tot("tail"), tot("exit"), tot("spin")))
    elif len(a) >= 3 and a[0] == "same":
        return same(a[1], a[2])
    else:
        print(__doc__)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
