#!/usr/bin/env python3
"""pair_codegen.py PARENT.s CHANGE.s -- code generation of the pair kernels, two trees side by side.

Both files are the device assembly of secedo_amd/csrc/simmat_kernels.hip (hipcc -S --cuda-device-only with the
Makefile's flags). Per instance of accumulate_counts / accumulate_masks / accumulate_tiles: registers, spills, scratch,
occupancy and the mnemonic histogram ("parent | change"), and for accumulate_counts the audit of its counted LDS waits
(the COUNTED WAITS comment in the kernel):
  * every hand-issued column-word load (an asm statement of ds_read2_b32 / ds_read_b32) and the hand-placed wait that
    consumes it; between the two no instruction that is not part of an asm statement may name a loaded register (a
    v_mov, a v_writelane, a scratch access: the data has not landed);
  * no scalar memory load behind the first hand-issued load (scalar loads share lgkmcnt and return out of order);
  * the compiler's own s_waitcnt lgkmcnt behind the first hand-issued load, counted, and how many of them lie directly
    between an item's unpacking and its slot block (a v_bfe / v_lshrrev of the item in front, ASMSTART behind).
"""
import collections
import re
import subprocess
import sys

CXXFILT = "c++filt"


def functions(path):
    text = open(path).read()
    meta = {}
    for m in re.finditer(r"  - \.agpr_count:.*?\n(?=  - \.agpr_count:|amdhsa\.target)", text, re.S):
        block = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", block)}
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        if "accumulate_" not in name or name not in meta:
            continue
        occ = re.search(r"; Occupancy: (\d+)", text[m.end():m.end() + 4000])
        out[name] = (body.split("\n"), meta[name], int(occ.group(1)) if occ else -1)
    names = subprocess.run([CXXFILT], input="\n".join(out), capture_output=True, text=True).stdout.split("\n")
    short = lambda n: re.sub(r"^void secedo::\(anonymous namespace\)::|\(secedo.*$", "", n)
    return {short(d): out[n] for n, d in zip(out, names)}


def mnemonic(line):
    m = re.match(r"\t([a-z]\w+)", line)
    return m.group(1) if m else None


def histogram(lines):
    return collections.Counter(filter(None, map(mnemonic, lines)))


def regs_of(operand):
    m = re.match(r"v\[(\d+):(\d+)\]", operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", operand)
    return {int(m.group(1))} if m else set()


def audit_waits(lines):
    in_asm, loads, pending, touched, first_load = False, 0, {}, [], None
    hand_waits, s_loads, compiler_waits, waits_before_block = collections.Counter(), 0, 0, 0
    last_compiler_wait = None
    for i, line in enumerate(lines):
        if "ASMSTART" in line:
            in_asm = True
            if last_compiler_wait is not None and first_load is not None:
                waits_before_block += 1
            continue
        if "ASMEND" in line:
            in_asm = False
            continue
        mn = mnemonic(line)
        if mn is None:
            continue
        ops = [o.strip() for o in line.split(None, 1)[1].split(",")] if len(line.split(None, 1)) > 1 else []
        if in_asm and mn in ("ds_read2_b32", "ds_read_b32"):
            loads += 1
            first_load = i if first_load is None else first_load
            for r in regs_of(ops[0]):
                pending[r] = i
            continue
        if in_asm and mn == "s_waitcnt":
            hand_waits[line.strip()] += 1
            pending = {}
            continue
        if in_asm:
            continue
        if first_load is not None:
            if mn.startswith("s_load") or mn.startswith("s_buffer_load"):
                s_loads += 1
            if mn == "s_waitcnt" and "lgkmcnt" in line:
                compiler_waits += 1
                last_compiler_wait = i
                if "lgkmcnt(0)" in line:
                    pending = {}  # (a full wait of the compiler's lands the hand-issued loads too)
                continue
            if mn.startswith("v_") or mn.startswith("s_") or mn.startswith("ds_") or mn.startswith("buffer_"):
                if not mn.startswith("s_waitcnt"):
                    last_compiler_wait = None if mn.startswith("v_") or mn.startswith("ds_") else last_compiler_wait
            named = set()
            for o in ops:
                named |= regs_of(o.split()[0] if o else o)
            hit = named & set(pending)
            if hit:
                touched.append("line %d: %s (loaded at line %d)" % (i, line.strip(), pending[min(hit)]))
    return loads, hand_waits, s_loads, compiler_waits, waits_before_block, touched


def main():
    parent, change = functions(sys.argv[1]), functions(sys.argv[2])
    keys = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
            "group_segment_fixed_size")
    labels = ("vgpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch_B", "static_lds_B")
    for name in sorted(change):
        print(name)
        cl, cm, cocc = change[name]
        if name not in parent:
            print("    parent: no such instance")
            continue
        pl, pm, pocc = parent[name]
        same = all(pm[k] == cm[k] for k in keys) and pocc == cocc
        print("    resources %s: %s occupancy=%d|%d" % ("EQUAL" if same else "DIFFER", " ".join(
            "%s=%d|%d" % (l, pm[k], cm[k]) for l, k in zip(labels, keys)), pocc, cocc))
        ph, ch = histogram(pl), histogram(cl)
        diff = ["%s %d>%d" % (k, ph[k], ch[k]) for k in sorted(set(ph) | set(ch)) if ph[k] != ch[k]]
        print("    instructions %d|%d: %s" % (sum(ph.values()), sum(ch.values()),
                                              "histogram EQUAL" if not diff else "differ: " + ", ".join(diff)))
        if name.startswith("accumulate_counts"):
            for tag, lines in (("parent", pl), ("change", cl)):
                loads, hw, s_loads, cw, before, touched = audit_waits(lines)
                print("    %s waits: hand-issued word loads %d; hand-placed waits {%s}; s_load behind the first load %d; "
                      "compiler's lgkmcnt waits behind it %d, of them directly in front of an asm statement %d; "
                      "word registers named between load and wait: %s" % (
                          tag, loads, ", ".join("%s x%d" % kv for kv in sorted(hw.items())), s_loads, cw, before,
                          "none" if not touched else "; ".join(touched)))


if __name__ == "__main__":
    main()
