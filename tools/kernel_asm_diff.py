#!/usr/bin/env python3
"""Compare two builds' device assembly kernel by kernel: instruction text, kernel descriptor (the resource line) and argument list.

    make -C modurl_gym_amd/csrc asm                      # in both trees: build/{cartpole,mountain_car,pendulum}.s
    tools/kernel_asm_diff.py OLD/build NEW/build          # directories, or single .s files

Every kernel of OLD is looked up in NEW by its mangled name; an empty trailing template parameter pack ("JE" closing the template arguments,
"DpT<k>_" closing the parameter types) is not part of the name for this purpose, and the kernel's own name is masked in its text.  Compared are (1) the function body from its label to its end label, with the
comments and the function-order-dependent numbers of local labels (.LBB<fn>_<bb>, .Lfunc_end<fn>) taken out, (2) the .amdhsa_kernel block, (3) the kernel's
.args entry of the code-object metadata.  Prints one line per file and per changed or missing kernel; exit status 1 if any OLD kernel changed.

    tools/kernel_asm_diff.py --by-text OLD/build NEW/build

pairs by content instead, for a change that renames kernels: every OLD kernel's masked (text, descriptor, arguments) triple must occur among NEW's, counted
with multiplicity; an OLD kernel without one is CHANGED.
"""
import collections
import os
import re
import sys


def plain(name):
    """The mangled name without an empty trailing template parameter pack."""
    if re.search(r"DpT\d*_$", name) and "JEEEv" in name:
        return re.sub(r"DpT\d*_$", "", name.replace("JEEEv", "EEv", 1))
    return name


def kernels(path):
    text = open(path).read()
    lines = text.split("\n")
    out = {}
    desc = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        desc[m.group(1)] = m.group(2)
    meta = {}
    md = text.find(".amdgpu_metadata")
    if md >= 0:
        # one YAML list entry per kernel: "  - .agpr_count ... .args: ... .name: <kernel> ... .symbol"
        for ent in re.split(r"^  - (?=\.agpr_count)", text[md:], flags=re.M)[1:]:
            # the list's last entry ends where the next top-level key (amdhsa.target) begins, and has no line end of its own
            ent = re.split(r"\n(?=\S)", ent, maxsplit=1)[0].rstrip("\n")
            assert ent.startswith(".agpr_count")
            nm = re.search(r"^\s+\.name:\s+(\S+)", ent, re.M)
            if nm:
                meta[nm.group(1)] = ent
    i = 0
    while i < len(lines):
        m = re.match(r"^(\S+):\s*; @\1\s*$", lines[i])
        if m and m.group(1) in desc:
            name = m.group(1)
            j = i + 1
            while j < len(lines) and not re.match(r"^\.Lfunc_end\d+:", lines[j]):
                j += 1
            body = "\n".join(lines[i:j])
            body = re.sub(r"[ \t]*;.*$", "", body, flags=re.M)   # comments carry function-order-dependent block numbers too
            body = re.sub(r"\.LBB\d+_", ".LBB_", body)
            body = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", body)
            out[plain(name)] = tuple(part.replace(name, "KERNEL") for part in (body, desc[name], meta.get(name, "")))
            i = j
        i += 1
    return out


def main():
    by_text = "--by-text" in sys.argv[1:]
    old, new = [a for a in sys.argv[1:] if a != "--by-text"]
    pairs = [(old, new)] if os.path.isfile(old) else [(os.path.join(old, f), os.path.join(new, f)) for f in sorted(os.listdir(old)) if f.endswith(".s")]
    compared = changed = 0
    for a, b in pairs:
        ka, kb = kernels(a), kernels(b)
        c = 0
        left = collections.Counter(kb.values())
        for name, parts in ka.items():
            compared += 1
            if by_text:
                if left[parts] == 0:
                    print(f"CHANGED  {name}: no kernel of the new build has its text, descriptor and arguments")
                    c += 1
                left[parts] -= 1
                continue
            if name not in kb:
                print(f"MISSING  {name}")
                c += 1
                continue
            what = [w for w, x, y in zip(("text", "descriptor", "arguments"), parts, kb[name]) if x != y]
            if what:
                print(f"CHANGED  {name}: {', '.join(what)}")
                c += 1
        changed += c
        print(f"{os.path.basename(a)}: {len(ka)} kernels of the old build compared, {c} changed; the new build has {len(kb) - (len(ka) - c if by_text else len(set(ka) & set(kb)))} more")
    print(f"total: {compared} compared, {changed} changed")
    sys.exit(1 if changed else 0)


if __name__ == "__main__":
    main()
