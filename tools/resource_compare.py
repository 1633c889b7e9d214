#!/usr/bin/env python3
"""Compare the kernel resource usage of two builds of the library.

    make -C <package> EXTRA=-Rpass-analysis=kernel-resource-usage 2> before.log      (one tree)
    make -C <package> EXTRA=-Rpass-analysis=kernel-resource-usage 2> after.log       (the other)
    tools/resource_compare.py before.log after.log [--show SUBSTRING ...] > profiles/<name>.txt

Every fused_round_rows instantiation present in both logs is compared on VGPRs, SGPRs, LDS, scratch,
waves per SIMD and SGPR / VGPR spills; the differing ones are listed (none: one line says so).  Instantiations whose demangled name
holds one of the --show substrings are printed in full, new ones included."""
import argparse
import collections
import re
import subprocess

FIELDS = (("VGPRs", "vgpr"), ("TotalSGPRs", "sgpr"), ("LDS Size [bytes/block]", "lds"),
          ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "waves"),
          ("SGPRs Spill", "sspill"), ("VGPRs Spill", "vspill"))


def parse(path):
    out, cur = collections.OrderedDict(), None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def demangle(names):
    if not names:
        return {}
    got = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, got.stdout.splitlines()))


def short(name):
    """fused_round_rows<Policy, NS, TW, NT, GROUPED, SP, ...> without the anonymous namespace and the tables"""
    name = name.replace("(anonymous namespace)::", "").replace("mx::fused::", "")
    m = re.match(r"void fused_round_rows<(.*?), (\d+), (\d+), (true|false), (true|false), (\d+)", name)
    if not m:
        return name
    pol, ns, tw, nt, grouped, sp = m.groups()
    return f"{pol:<28} {ns:>2} x {tw} nt={nt[0]} grouped={grouped[0]} sp={sp}"


def row(r):
    return "  ".join(f"{k}={r.get(k, '?'):>5}" for _, k in FIELDS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--show", nargs="*", default=[])
    a = ap.parse_args()
    before, after = parse(a.before), parse(a.after)
    names = demangle(sorted(set(before) | set(after)))
    fused = [n for n in after if "fused_round_rows" in names[n]]
    both = [n for n in fused if n in before]
    differ = [n for n in both if before[n] != after[n]]
    print(f"fused_round_rows instantiations: {sum('fused_round_rows' in names[n] for n in before)} before, "
          f"{len(fused)} after, {len(both)} in both")
    other = [n for n in after if n in before and n not in fused]
    other_differ = [n for n in other if before[n] != after[n]]
    print(f"other kernels in both builds: {len(other)}, of which {len(other_differ)} differ")
    if not differ:
        print("every instantiation present in both builds: VGPRs, SGPRs, LDS, scratch, waves per SIMD and spills unchanged")
    for n in differ + other_differ:
        print("CHANGED", short(names[n]))
        print("   before", row(before[n]))
        print("   after ", row(after[n]))
    for sub in a.show:
        print(f"\n-- instantiations matching '{sub}' (after; '*' = not in the before build)")
        for n in fused:
            if sub in names[n].replace("(anonymous namespace)::", ""):
                print(("* " if n not in before else "  ") + short(names[n]), " ", row(after[n]))


if __name__ == "__main__":
    main()
