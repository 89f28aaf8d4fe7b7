"""Compare the gfx950 kernels of two builds instruction by instruction (a refactor's "same machine code" check).

Build both trees with the Makefile's flags plus -save-temps=obj, then

    python scripts/kernel_isa_diff.py PARENT_OBJ BRANCH_OBJ --units mlp_gemm mlp_fwd_stream rollout_mlp \
        --out profiles/gemm_split_isa.json

Every kernel of the named units of PARENT_OBJ is looked up in whichever unit of BRANCH_OBJ emits it now and compared:
  * the instruction text: comments and blank lines dropped, the function number in .LBB<n>_ / .LJTI<n>_ / .Lfunc_end<n>
    labels dropped, the kernel's own symbol replaced by a placeholder;
  * the kernel descriptor (.amdhsa_* directives) and the code-object metadata: agpr / vgpr / sgpr counts, LDS bytes,
    scratch bytes, spill counts.
Kernels are matched by demangled name with "(anonymous namespace)::" removed, so a parameter type that moved between
an anonymous and a named namespace still matches.  A kernel that gained a template parameter is found under its new
name with --rename PATTERN=REPLACEMENT (a regular expression applied to the parent's demangled names), e.g.
--rename 'lstm_cell_bwd_kernel\(=lstm_cell_bwd_kernel<256>('.  Exit status 1 if a kernel is missing or differs."""

import argparse
import glob
import json
import os
import re
import subprocess
import sys

META = ("agpr_count", "vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "sgpr_spill_count", "vgpr_spill_count")


def demangle(symbols, cxxfilt):
    out = subprocess.run([cxxfilt], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout
    return [s.replace("(anonymous namespace)::", "") for s in out.split("\n")[:len(symbols)]]


def normalise(lines, symbol):
    text = []
    for ln in lines:
        s = ln.split(";")[0].strip()  # comments: whole lines and the tails of label / instruction lines
        if not s:
            continue
        s = re.sub(r"\.(LBB|LJTI|Lfunc_end|Lfunc_begin)\d+", r".\1", s.replace(symbol, "<kernel>"))
        text.append(re.sub(r"\s+", " ", s))
    return text


def kernels_of(path):
    """{symbol: {"unit", "text", "descriptor", "meta"}} of one device assembly file"""
    lines = open(path).read().split("\n")
    unit = os.path.basename(path).split("-hip-")[0]
    found, i = {}, 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if not m:
            i += 1
            continue
        sym = m.group(1)
        end = next(j for j in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[j])
        start = max(j for j in range(i) if lines[j].startswith(sym + ":"))
        found[sym] = {"unit": unit, "text": normalise(lines[start + 1:i], sym),
                      "descriptor": normalise(lines[i + 1:end], sym), "meta": {}}
        i = end + 1
    block = None
    for ln in lines:  # the code-object metadata (YAML): kernel-level keys sit at four spaces
        if ln.startswith("  - "):
            block = {}
            ln = "    " + ln[4:]
        m = re.match(r"    \.(\w+):\s+(\S+)", ln)
        if block is not None and m:
            block[m.group(1)] = m.group(2)
            if m.group(1) == "name" and m.group(2) in found:
                found[m.group(2)]["meta"] = block
    for k in found.values():
        k["meta"] = {key: int(k["meta"][key]) for key in META if key in k["meta"]}
    return found


def load(obj_dir, units):
    out = {}
    for path in sorted(glob.glob(os.path.join(obj_dir, "*-hip-amdgcn-amd-amdhsa-gfx950.s"))):
        if units is None or os.path.basename(path).split("-hip-")[0] in units:
            out.update(kernels_of(path))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent_obj")
    ap.add_argument("branch_obj")
    ap.add_argument("--units", nargs="+", required=True, help="units of the parent whose kernels are compared")
    ap.add_argument("--cxxfilt", default="c++filt")
    ap.add_argument("--rename", nargs="*", default=[], metavar="PATTERN=REPLACEMENT",
                    help="rewrite the parent's demangled kernel names before the lookup")
    ap.add_argument("--out")
    a = ap.parse_args()
    parent, branch = load(a.parent_obj, set(a.units)), load(a.branch_obj, None)
    pnames = demangle(list(parent), a.cxxfilt)
    for rule in a.rename:
        pat, rep = rule.split("=", 1)
        pnames = [re.sub(pat, rep, n) for n in pnames]
    pname = dict(zip(pnames, parent.values()))
    bname = dict(zip(demangle(list(branch), a.cxxfilt), branch.values()))
    missing, differ, moved = [], [], {}
    for name, p in sorted(pname.items()):
        b = bname.get(name)
        if b is None:
            missing.append(name)
            continue
        moved.setdefault(f"{p['unit']} -> {b['unit']}", 0)
        moved[f"{p['unit']} -> {b['unit']}"] += 1
        what = [k for k in ("text", "descriptor", "meta") if p[k] != b[k]]
        if what:
            differ.append({"kernel": name, "differs_in": what, "parent_meta": p["meta"], "branch_meta": b["meta"]})
    result = {"parent_units": sorted(a.units), "kernels": len(pname), "identical": len(pname) - len(missing) - len(differ),
              "missing": missing, "differ": differ, "emitted_by": moved, "renamed": a.rename,
              "compared": "instruction text, .amdhsa_* descriptor, metadata " + ", ".join(META)}
    print(json.dumps(result, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 1 if missing or differ else 0


if __name__ == "__main__":
    sys.exit(main())
