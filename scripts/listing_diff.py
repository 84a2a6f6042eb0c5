#!/usr/bin/env python3
"""Does a refactor leave hipcc's device code as it was?  Compiles one source file of two csrc trees with the Makefile's flags
plus `-S --cuda-device-only` and compares the listings function by function.

    scripts/listing_diff.py PARENT_CSRC NEW_CSRC FILE.hip [--rename OLD=NEW ...]

One line per `revo::` device function: SAME, or DIFF with both line counts; exit status 1 on any DIFF and on a function
that only one tree has.  A listing is the function's text from its label to its end label plus its kernel descriptor
(`.amdhsa_kernel` block: registers, scratch, LDS).  Before the comparison, and nothing else:
  * every `_ZN4revo...` symbol (the function's own name, the functions it calls) is replaced by its demangled name, the
    parent's after the renames;
  * basic-block labels `.LBBn_m` lose the function's number n;
  * the `__hip_cuid_...` symbol loses its hash.
--rename takes a regular expression and its replacement (re.sub on the parent's demangled names, in the order given), for
functions the refactor renamed, e.g.  'topk_scan256_filtered_kernel<(.*?)>=topk_scan256_kernel<\\1, true>'.
The script compares text; it does not look at what the instructions are."""
import argparse
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = os.environ.get("CXXFILT") or shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
_SYM = re.compile(r"\b_ZZ?N(?:K?)4revo\w+")


def makefile_flags(csrc):
    """CXXFLAGS of csrc/Makefile with $(ARCH) filled in."""
    text = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, flags=re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, flags=re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def listing(csrc, src, out):
    cmd = [HIPCC, *makefile_flags(csrc), "-S", "--cuda-device-only", src, "-o", out]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"{' '.join(cmd)} (in {csrc}) failed:\n{r.stderr[-3000:]}")
    return open(out).read()


def demangle(names):
    names = sorted(names)
    if not names:
        return {}
    if not CXXFILT:
        sys.exit("no demangler: put llvm-cxxfilt or c++filt on PATH, or set CXXFILT")
    r = subprocess.run([CXXFILT], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def functions(asm, renames):
    """{demangled (and renamed) name: normalised lines} of the revo:: functions of one listing."""
    names = demangle(set(_SYM.findall(asm)))
    for k, v in names.items():
        for pat, repl in renames:
            v = re.sub(pat, repl, v)
        names[k] = v

    def norm(text):
        text = _SYM.sub(lambda m: "{" + names[m.group(0)] + "}", text)
        text = re.sub(r"\.LBB\d+_", ".LBB_", text)
        return re.sub(r"__hip_cuid_\w+", "__hip_cuid", text).splitlines()

    out = {}
    for m in re.finditer(r"^(_ZZ?NK?4revo\w+):\s*(?:;.*)?$", asm, flags=re.M):
        sym = m.group(1)
        body = asm[m.start(): asm.index(".Lfunc_end", m.end())]
        d = re.search(r"^\s*\.amdhsa_kernel " + re.escape(sym) + r"\n.*?^\s*\.end_amdhsa_kernel", asm, flags=re.M | re.S)
        out[names[sym]] = norm(body) + (norm(d.group(0)) if d else [])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent_csrc")
    ap.add_argument("new_csrc")
    ap.add_argument("file")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    a = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in a.rename]
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(2) as ex:
        old = ex.submit(listing, os.path.abspath(a.parent_csrc), a.file, os.path.join(tmp, "parent.s"))
        new = ex.submit(listing, os.path.abspath(a.new_csrc), a.file, os.path.join(tmp, "new.s"))
        old, new = functions(old.result(), renames), functions(new.result(), [])
    same = bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"{'ONLY NEW' if name in new else 'ONLY PARENT'}  {name}")
            bad += 1
        elif old[name] == new[name]:
            print(f"SAME  {name}")
            same += 1
        else:
            print(f"DIFF  {len(old[name])} -> {len(new[name])} lines  {name}")
            bad += 1
    print(f"{a.file}: {same} SAME, {bad} DIFF or unmatched")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
