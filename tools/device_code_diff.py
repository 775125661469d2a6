"""Device code of two trees, kernel by kernel:  python tools/device_code_diff.py --against PARENT_TREE [--jobs N] [hipcc flags...]
The proof that a host-side change left every kernel alone; needs no GPU.  For every unit in the Makefile's SRC of either tree: compile with the Makefile's
flags plus --cuda-device-only -S (and the flags given here, e.g. -DHSRLE_EXPERIMENTS), cut the assembly at the function symbols (a kernel's text with its
.amdhsa_kernel block: registers, LDS, scratch), strip ; comments and trailing blanks, and take the function number out of the local labels (.LBB<n>_ -> .LBB_,
.Lfunc_end<n>, .Ltmp<n>, .LJTI<n>_ likewise: a unit that defines its kernels in another order numbers them differently).  Prints a markdown summary -- kernels per
unit, added, removed, changed, and the k_decode_blocks instantiations -- and exits 1 if any kernel was added, removed or changed.
    git worktree add ../parent HEAD~1 && python tools/device_code_diff.py --against ../parent"""
import concurrent.futures, os, re, subprocess, sys, tempfile

PKG = "hypersonic-rle-kit_amd"
LABEL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp|LJTI)\d+")


def makefile_vars(tree):
    """SRC units and the compile flags, read from the tree's Makefile"""
    text = open(os.path.join(tree, PKG, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, text, re.M).group(1)
    flags = var("CXXFLAGS").replace("$(ARCH)", var("ARCH")).split()
    return var("SRC").split(), var("HIPCC"), flags


def compile_unit(tree, unit, hipcc, flags, out):
    cmd = [hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(tree, PKG, unit), "-o", out]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, timeout=3600)
    if r.returncode != 0:
        sys.exit("%s of %s does not compile:\n%s" % (unit, tree, r.stderr[-4000:]))
    return out


def functions_of(path):
    """{symbol: normalised text} of every function of an assembly file, from its label to its .size line"""
    funcs, name, body = {}, None, []
    for line in open(path):
        if name is None:
            m = re.match(r"\s*\.type\s+([\w.$]+),@function", line)
            if m:
                name, body = m.group(1), []
            continue
        line = LABEL.sub(lambda m: "." + m.group(1), line.split(";", 1)[0].rstrip())
        if line:
            body.append(line)
        if re.match(r"\s*\.size\s+" + re.escape(name) + ",", line):
            funcs[name] = "\n".join(body)
            name = None
    return funcs


def main():
    argv = sys.argv[1:]
    if "--against" not in argv:
        sys.exit(__doc__)
    i = argv.index("--against")
    other = os.path.abspath(argv[i + 1])
    del argv[i : i + 2]
    jobs = 8
    if "--jobs" in argv:
        i = argv.index("--jobs")
        jobs = int(argv[i + 1])
        del argv[i : i + 2]
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    trees = {"here": here, "against": other}
    with tempfile.TemporaryDirectory() as tmp:
        work = []
        for tag, tree in trees.items():
            src, hipcc, flags = makefile_vars(tree)
            for unit in src:
                work.append((tag, unit, tree, hipcc, flags + argv, os.path.join(tmp, tag + "_" + os.path.basename(unit) + ".s")))
        with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as pool:
            outs = list(pool.map(lambda w: compile_unit(w[2], w[1], *w[3:]), work))
        code = {"here": {}, "against": {}}   # [tag][unit] = {symbol: text}
        for (tag, unit, *_), out in zip(work, outs):
            code[tag][unit] = functions_of(out)

    units = list(dict.fromkeys([w[1] for w in work]))
    total = {"here": 0, "against": 0, "added": 0, "removed": 0, "changed": 0, "dec_here": 0, "dec_against": 0}
    details = []
    print("flags beyond the Makefile's: %s\n" % (" ".join(argv) or "none"))
    print("| unit | functions here | against | added | removed | changed | k_decode_blocks here | against |")
    print("|---|---:|---:|---:|---:|---:|---:|---:|")
    for unit in units:
        a, b = code["here"].get(unit), code["against"].get(unit)
        fa, fb = a or {}, b or {}
        added, removed = sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa))
        changed = sorted(k for k in fa if k in fb and fa[k] != fb[k])
        dec = [sum("k_decode_blocks" in k for k in f) for f in (fa, fb)]
        print("| %s | %s | %s | %d | %d | %d | %d | %d |" % (unit, len(fa) if a is not None else "(no such unit)", len(fb) if b is not None else "(no such unit)", len(added),
                                                             len(removed), len(changed), dec[0], dec[1]))
        for key, n in (("here", len(fa)), ("against", len(fb)), ("added", len(added)), ("removed", len(removed)), ("changed", len(changed)), ("dec_here", dec[0]),
                       ("dec_against", dec[1])):
            total[key] += n
        details += ["%s: %s %s" % (unit, what, k) for what, ks in (("added", added), ("removed", removed), ("changed", changed)) for k in ks]
    print("\n%d functions here, %d against; added %d, removed %d, changed %d; k_decode_blocks instantiations %d here, %d against"
          % (total["here"], total["against"], total["added"], total["removed"], total["changed"], total["dec_here"], total["dec_against"]))
    for d in details:
        print(d)
    sys.exit(1 if details else 0)


if __name__ == "__main__":
    main()
