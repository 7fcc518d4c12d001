#!/usr/bin/env python
"""Are two csrc trees the same device code?  python scripts/isa_same.py OLD_CSRC NEW_CSRC [file.hip ...]

Development aid for refactors of the kernels: compiles every named file (default: the Makefile's SRCS) of both trees to gfx950
assembly with the Makefile's FLAGS plus --cuda-device-only -S, once plain and once with -DPMN_EXPERIMENTAL, drops what names the
compilation rather than the code (comment lines, .file, .ident, the __hip_cuid_ symbol), cuts each listing at its kernel symbols
(body, .amdhsa_kernel block = register / LDS / scratch budget) and prints one line per kernel: same, or DIFFERENT (n lines).  Text
comparison only.  Exit status 1 on any difference.  Both trees must sit where their own #include "../../include/pmn_hip.h" resolves
(e.g. `git archive <commit> patchmatchnet_amd/csrc include | tar -x -C /tmp/old`)."""
import concurrent.futures, difflib, os, re, shutil, subprocess, sys, tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def makefile_vars(csrc):
    text = open(os.path.join(csrc, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, text, re.M).group(1).strip()
    return var("FLAGS").replace("$(ARCH)", var("ARCH")).split(), var("SRCS").split()


def listing(csrc, name, flags, extra, out):
    cmd = [HIPCC] + flags + extra + ["--cuda-device-only", "-S", name, "-o", out]
    subprocess.run(cmd, cwd=csrc, check=True, stderr=subprocess.PIPE)
    lines = []
    for line in open(out):
        s = line.strip()
        if not s or s.startswith(";") or s.startswith(".file") or s.startswith(".ident") or "__hip_cuid_" in s:
            continue
        lines.append(line.rstrip())
    return lines


def by_kernel(lines):
    """{section: [lines]} -- a kernel's section is its body (label .. .Lfunc_end) plus its .amdhsa_kernel block; the rest (device
    functions that were not inlined, the metadata note) goes under "(rest)"."""
    kernels = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m}
    parts, cur = {"(rest)": []}, "(rest)"
    for l in lines:
        m = re.match(r"(\S+):", l)
        if m and m.group(1) in kernels:
            cur = m.group(1)
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            cur = m.group(1)
        parts.setdefault(cur, []).append(l)
        if l.startswith(".Lfunc_end") or l.strip() == ".end_amdhsa_kernel":
            cur = "(rest)"
    return parts


def demangle(names):
    # the toolchain's own demangler first: binutils' c++filt does not know _Float16 (DF16_) and leaves those kernels mangled
    beside = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "llvm", "bin", "llvm-cxxfilt")
    tool = (beside if os.path.exists(beside) else None) or shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        return {n: n for n in names}
    # (where only binutils' is there: hand it _Float16 as the half type it knows, Dh, and put the name back)
    half = "llvm" not in os.path.basename(tool)
    text = "\n".join(n.replace("DF16_", "Dh") if half else n for n in names)
    out = subprocess.run([tool], input=text, capture_output=True, text=True).stdout.replace("__fp16", "_Float16").split("\n")
    return {n: re.sub(r"(?<=.)\(.*", "", d).replace("void ", "") for n, d in zip(names, out)}


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    old, new = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    flags, srcs = makefile_vars(new)
    files = sys.argv[3:] or srcs
    builds = [("plain", []), ("experimental", ["-DPMN_EXPERIMENTAL"])]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        jobs = {(f, b, t): pool.submit(listing, t, f, flags, x, os.path.join(tmp, "%d.s" % i))
                for i, (f, (b, x), t) in enumerate((f, bx, t) for f in files for bx in builds for t in (old, new))}
        for f in files:
            for b, _ in builds:
                a, c = by_kernel(jobs[f, b, old].result()), by_kernel(jobs[f, b, new].result())
                names = demangle(sorted(set(a) | set(c)))
                for k in sorted(names):
                    n = 0
                    if a.get(k) != c.get(k):
                        diff = difflib.unified_diff(a.get(k, []), c.get(k, []), n=0, lineterm="")
                        n = sum(1 for d in diff if d[:1] in "+-" and d[:3] not in ("+++", "---"))
                    bad += n > 0
                    print("%-14s %-12s %-9s %s" % (f, b, "same" if not n else "DIFFERENT (%d lines)" % n, names[k]))
    print("%d section(s) differ" % bad if bad else "all sections identical")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
