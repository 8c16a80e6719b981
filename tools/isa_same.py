#!/usr/bin/env python3
"""Are the kernels of two device-assembly files (hipcc --offload-device-only -S) the same machine code?
tools/isa_same.py OLD.s NEW.s [--sub REGEX REPL]...

Kernels are paired by demangled name; each --sub rewrites the OLD names first (a refactor that drops or
renumbers a template argument).  A pair is identical when three texts agree once the kernel's own mangled
name and the function index of local labels (.LBB<n>_, .Lfunc_end<n>, ...) are normalised: the code from the
kernel's label to its .Lfunc_end (without the assembler's comments, which carry function indices too and move
when a unit gains or loses a kernel), the .amdhsa_kernel descriptor, and the kernel's metadata entry (register,
spill, LDS and scratch figures).  Prints one line per kernel - name, instruction count, identical yes / no -
and the first differing lines of a pair that is not; exit status 1 if any pair differs or is unpaired.
tools/isa_mix.py shows the opcode mix of a differing pair."""
import re
import shutil
import subprocess
import sys


def demangle(names):
    cxxfilt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "x86_64-linux-gnu-c++filt"
    r = subprocess.run([cxxfilt], input="\n".join(names) + "\n", capture_output=True,
                       text=True, check=True)
    return r.stdout.split("\n")[:len(names)]


def kernels(path):
    """{mangled name: (code lines, descriptor lines, metadata lines)}, names replaced by KERNEL"""
    s = open(path).read()
    names = re.findall(r"^\t\.amdhsa_kernel (\S+)$", s, re.M)
    meta = s[s.index(".amdgpu_metadata"):s.index(".end_amdgpu_metadata")]
    entries = re.split(r"^  - (?=\.agpr_count)", meta, flags=re.M)[1:]
    out = {}
    for n in names:
        i = s.index("\n" + n + ":")
        code = s[i:s.index(".Lfunc_end", i)]
        j = s.index("\t.amdhsa_kernel " + n + "\n")
        desc = s[j:s.index(".end_amdhsa_kernel", j)]
        (ent,) = [e for e in entries if re.search(r"^    \.name: +" + re.escape(n) + "$", e, re.M)]
        texts = []
        code = re.sub(r"[ \t]*;.*", "", code)  # assembler comments name other blocks by function index (BB<n>_<k>)
        for t in (code, desc, ent):
            t = t.replace(n, "KERNEL")
            t = re.sub(r"\.L([A-Za-z_]+?)(\d+)(_\d+)?\b", lambda m: ".L" + m.group(1) + "N" + (m.group(3) or ""), t)
            texts.append(t.splitlines())
        out[n] = texts
    return out


def n_instructions(code):
    return sum(1 for l in code if l.startswith("\t") and not l.strip().startswith((".", ";")))


def main(argv):
    subs = []
    while "--sub" in argv:
        i = argv.index("--sub")
        subs.append((argv[i + 1], argv[i + 2]))
        del argv[i:i + 3]
    old, new = kernels(argv[1]), kernels(argv[2])
    on = dict(zip(demangle(list(old)), old))
    nn = dict(zip(demangle(list(new)), new))
    for pat, repl in subs:
        on = {re.sub(pat, repl, k): v for k, v in on.items()}
    bad = same_pairs = 0
    print(f"{argv[1]} ({len(old)} kernels) -> {argv[2]} ({len(new)} kernels)")
    for name in sorted(set(on) | set(nn)):
        if name not in on or name not in nn:
            print(f"{name}: only in {'NEW' if name in nn else 'OLD'}")
            bad += 1
            continue
        a, b = old[on[name]], new[nn[name]]
        same = a == b
        print(f"{name}: instructions {n_instructions(a[0])} {n_instructions(b[0])} identical {'yes' if same else 'NO'}")
        same_pairs += same
        if not same:
            bad += 1
            for what, x, y in zip(("code", "descriptor", "metadata"), a, b):
                diff = [(p, q) for p, q in zip(x, y) if p != q][:5]
                if len(x) != len(y):
                    print(f"  {what}: {len(x)} lines -> {len(y)}")
                for p, q in diff:
                    print(f"  {what}: {p.strip()}  ->  {q.strip()}")
    print(f"{same_pairs} of {len(set(on) | set(nn))} kernels identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(list(sys.argv)))
