#!/usr/bin/env python3
"""Build-time check of the hand-written matrix-instruction streams (kge_rank_screen_r.h and friends).

gfx90a+ wants two wait states between a VALU write of a VGPR and a matrix instruction that reads it as a source (LLVM's
GCNHazardRecognizer inserts them for its own matrix instructions: LegacyVALUWritesVGPRWaitStates).  The screening kernels issue their
v_mfma as inline assembly, where the compiler can neither see the instruction nor pad it -- a register-allocator copy (v_mov /
v_accvgpr_read of a parked fragment) placed right in front of such a statement makes the matrix instruction read a stale register:
wrong, timing-dependent results (round 6: profiles/r06y2_*).  This script reads the device assembly of every ranking unit
(ampligraph_amd/csrc/kge_rank*.hip) and fails if any v_mfma has a non-matrix VALU write to one of its VGPR sources within the two
instructions in front of it.  The assembly comes from the Makefile's `rank-asm` target: the library's own flags, architecture and
EXTRA, one compile per unit, in parallel.

usage: check_mfma_hazards.py [file.s ...]   (assembly files only; default: `make rank-asm` and every unit it lists); exit code 1 on a hit."""
import os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def regs(tok):
    tok = tok.strip(",")
    m = re.match(r"v\[(\d+):(\d+)\]$", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", tok)
    return {int(m.group(1))} if m else set()


def scan(asm_text):
    """-> list of (kernel, wait states in between, writer, mfma)"""
    hits, kernel, window = [], "?", []   # window: (instruction text, wait states it provides)
    for raw in asm_text.split("\n"):
        l = raw.split(";")[0].strip()
        if not l or l.startswith("."):
            continue
        m = re.match(r"^(\S+):$", l)
        if m:
            if m.group(1).startswith("_Z"):
                kernel, window = m.group(1), []
            continue   # (a label between the copy and the matrix instruction does not add a wait state)
        toks = re.split(r"[ ,]+", l)
        op = toks[0]
        if op.startswith("v_mfma") or op.startswith("v_smfmac"):
            src = set()
            for t in toks[2:5]:
                src |= regs(t)
            between = 0
            for w, ws in reversed(window[-4:]):
                if between >= 2:
                    break
                wt = re.split(r"[ ,]+", w)
                if wt[0].startswith("v_") and not wt[0].startswith(("v_mfma", "v_smfmac", "v_cmp", "v_readlane", "v_readfirstlane")) and len(wt) > 1 and regs(wt[1]) & src:
                    hits.append((kernel, between, w, l))
                between += ws
        window.append((l, int(toks[1]) + 1 if op == "s_nop" and len(toks) > 1 and toks[1].isdigit() else 1))
        window = window[-8:]
    return hits


def unit_asm(asmdir=None):
    """{unit: device assembly text} of the ranking units (the Makefile's RANK_SRCS), through `make rank-asm` (up to date units are
    not compiled again)."""
    csrc = os.path.join(ROOT, "ampligraph_amd", "csrc")
    asmdir = asmdir or os.path.join(ROOT, "build", "obj", "asm")
    # MAX_JOBS when set, else the CPUs this process may use, at most 16 (as build() does)
    jobs = os.environ.get("MAX_JOBS") or str(min(16, len(os.sched_getaffinity(0))))
    r = subprocess.run(["make", "-C", csrc, "-j", jobs, "rank-asm", "ASMDIR=" + asmdir], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    if r.returncode:   # (the compiler's own words; a clean compile's warnings are the library build's to show)
        sys.stderr.write(r.stderr)
        raise subprocess.CalledProcessError(r.returncode, r.args)
    units = subprocess.run(["make", "-s", "-C", csrc, "print-rank-srcs"], check=True, capture_output=True, text=True).stdout.split()
    return {u: open(os.path.join(asmdir, u[:-4] + ".s")).read() for u in units}


def device_asm(path=None):
    """The device assembly of evaluate() as ONE text: every ranking unit's, whichever of them `path` names (callers that knew the
    ranking code as the single file kge_rank.hip name that one)."""
    asm = unit_asm()
    if path is not None and os.path.basename(path) not in asm:
        raise ValueError("%s is not a ranking unit (%s)" % (path, ", ".join(asm)))
    return "\n".join(asm.values())


def main(argv):
    other = [f for f in argv[1:] if not f.endswith(".s")]
    if other:
        print("not assembly files: %s (sources are compiled by `make rank-asm`: run without arguments)" % " ".join(other))
        return 2
    texts = {f: open(f).read() for f in argv[1:]} or unit_asm()
    bad = 0
    for f, text in texts.items():
        hits = scan(text)
        n = len(re.findall(r"^\s*v_mfma", text, re.M))
        print("%s: %d matrix instructions, %d with a VALU write of a source inside two wait states" % (os.path.basename(f), n, len(hits)))
        for k, d, w, m in hits[:20]:
            print("  %s: %d wait state(s) between: %s  ->  %s" % (k[:60], d, w, m))
        bad += len(hits)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
