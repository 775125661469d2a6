"""Registers, LDS and occupancy of every k_decode_blocks instantiation:  python tools/decode_resources.py [--csv] [--against FILE] [hipcc flags...]
Compiles every decoder translation unit (csrc/inst_w*.hip) for gfx950 to assembly (-S, device side only; needs no GPU) and prints one markdown table row per
instantiation: NumVgprs, LDS bytes, the compiler's occupancy (waves per SIMD by registers) and the waves per CU that LDS allows (160 KiB per CU).
The guard rail of changes to hsrle_decode.hip.h and of every toolchain change: no instantiation may lose a wave per SIMD.  --csv prints comma
separated rows.  --against FILE (a --csv output of another tree or toolchain, e.g. the parent's) prints the two joined per instantiation with a summary -- the form of
profiles/r09_decode_resources.md -- and exits 1 if an instantiation lost a wave per SIMD, changed its LDS or gained scratch:
    git worktree add ../parent HEAD~1 && python ../parent/tools/decode_resources.py --csv > parent.csv && python tools/decode_resources.py --against parent.csv"""
import concurrent.futures, os, re, subprocess, sys, tempfile

repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
csrc = os.path.join(repo, "hypersonic-rle-kit_amd", "csrc")
argv = sys.argv[1:]
against = None
if "--against" in argv:
    i = argv.index("--against")
    against = argv[i + 1]
    del argv[i : i + 2]
flags = [a for a in argv if a != "--csv"]
csv = "--csv" in argv
units = ["inst_w8", "inst_w16", "inst_w24", "inst_w32", "inst_w48", "inst_w64", "inst_w128"]
FAMILIES = {0: "PLAIN", 1: "PACKED", 2: "LUT3", 3: "LUT7", 4: "SINGLE", 5: "PACKED_SINGLE", 6: "SHORT0", 7: "SHORT1", 8: "SHORT3", 9: "SHORT7", 10: "SHORT_SINGLE"}
LDS_PER_CU = 160 * 1024


def compile_unit(unit, tmp):
    out = os.path.join(tmp, unit + ".s")
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I" + csrc, "-I" + os.path.join(repo, "include"),
           os.path.join(csrc, unit + ".hip"), "-o", out] + flags
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, timeout=1800)
    if r.returncode != 0:
        sys.exit("%s does not compile:\n%s" % (unit, r.stderr[-4000:]))
    return unit, out


def family_names():
    """The FAM enumerators of hsrle_codecs.h / hsrle_common.hip.h by value, if they can be read from the source; else the numbers."""
    names = {}
    for f in ("hsrle_codecs.h", "hsrle_common.hip.h", "hsrle_decode.hip.h"):
        m = re.search(r"enum\s+(?:Family\s*)?(?::\s*\w+\s*)?\{([^}]*\bPLAIN\b[^}]*)\}", open(os.path.join(csrc, f)).read())
        if m:
            v = 0
            for item in re.sub(r"//[^\n]*", "", m.group(1)).split(","):
                item = item.strip()
                if not item:
                    continue
                if "=" in item:
                    item, val = [x.strip() for x in item.split("=")]
                    v = int(val, 0)
                names[v] = item
                v += 1
            return names
    return {}


def rows_of(unit, path, fam):
    """(unit, template arguments, vgprs, lds, occupancy) of every k_decode_blocks kernel in the assembly file"""
    rows, name = [], None
    for line in open(path):
        m = re.match(r"(_ZN5hsrle15k_decode_blocksI(\w+?)EEv\w*):", line)
        if m:
            args = re.findall(r"L[ib](\d+)E", m.group(2))
            name, cur = m.group(1), {"args": [int(a) for a in args]}
            continue
        if name is None:
            continue
        for key, pat in (("vgprs", r"; NumVgprs: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"), ("occ", r"; Occupancy: (\d+)"), ("scratch", r"; ScratchSize: (\d+)")):
            m = re.match(pat, line)
            if m:
                cur[key] = int(m.group(1))
        if "lds" in cur and "vgprs" in cur and "occ" in cur:
            a = cur["args"] + [1, 1, 0][len(cur["args"]) - 6:] if len(cur["args"]) < 9 else cur["args"]
            label = "<%s, S %d, AL %d, T %d, R %d, Q %d%s%s%s>" % (fam.get(a[0], str(a[0])), a[1], a[2], a[3], a[4], a[5], ", SGL" if a[6] else "", "" if a[7] else ", no ENT",
                                                                 ", WIN" if a[8] else "")
            rows.append((unit, label, cur["vgprs"], cur["lds"], cur["occ"], cur.get("scratch", 0)))
            name = None
    return rows


with tempfile.TemporaryDirectory() as tmp:
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(units), 8)) as pool:
        files = dict(pool.map(lambda u: compile_unit(u, tmp), units))
    fam = family_names() or FAMILIES
    rows = [r for u in units for r in rows_of(u, files[u], fam)]

def read_csv(path):
    """{(unit, instantiation): (vgprs, lds, waves per SIMD, waves per CU by LDS, scratch)} of a --csv output"""
    old = {}
    for line in open(path):
        m = re.match(r'(\w+),"(.*)",(\d+),(\d+),(\d+),(\d+),(\d+)', line)
        if m:
            old[(m.group(1), m.group(2))] = tuple(int(x) for x in m.groups()[2:])
    return old


if against is not None:
    old = read_csv(against)
    now = {(u, l): (v, lds, occ, LDS_PER_CU // lds if lds else 0, s) for u, l, v, lds, occ, s in rows}
    both = [k for k in now if k in old]
    lost = [k for k in both if now[k][2] < old[k][2] or now[k][1] != old[k][1] or now[k][4] > old[k][4]]
    changed = [k for k in both if now[k][0] != old[k][0]]
    print("%d instantiations (%d only here, %d only in %s); lost a wave per SIMD, changed LDS or gained scratch: %d; VGPR count changed: %d\n"
          % (len(now), len(now) - len(both), len(old) - len(both), os.path.basename(against), len(lost), len(changed)))
    print("| unit | k_decode_blocks | VGPRs before | VGPRs now | waves / SIMD before | now | LDS bytes | waves / CU (LDS) | scratch |")
    print("|---|---|---:|---:|---:|---:|---:|---:|---:|")
    for k in now:
        y, x = now[k], old.get(k)
        print("| %s | `%s` | %s | %d | %s | %d | %d | %d | %d |%s" % (k[0], k[1], x[0] if x else "-", y[0], x[2] if x else "-", y[2], y[1], y[3], y[4], "  <-- LOST" if k in lost else ""))
    sys.exit(1 if lost else 0)

if csv:
    print("unit,instantiation,vgprs,lds_bytes,waves_per_simd_by_registers,waves_per_cu_by_lds,scratch")
else:
    print("| unit | k_decode_blocks | VGPRs | LDS bytes | waves / SIMD (registers) | waves / CU (LDS) | scratch |")
    print("|---|---|---:|---:|---:|---:|---:|")
for unit, label, vgprs, lds, occ, scratch in rows:
    by_lds = LDS_PER_CU // lds if lds else 0
    if csv:
        print('%s,"%s",%d,%d,%d,%d,%d' % (unit, label, vgprs, lds, occ, by_lds, scratch))
    else:
        print("| %s | `%s` | %d | %d | %d | %d | %d |" % (unit, label, vgprs, lds, occ, by_lds, scratch))
print("\n%d instantiations" % len(rows))
