"""What the compiler made of every kernel, read without a GPU.  Each device translation unit of fast-dnn_amd/csrc is compiled
to assembly (hipcc --cuda-device-only -S) with exactly the flags csrc/Makefile gives that file -- they are taken from
`make -n`, not restated here -- and one line per kernel is printed: the code object's metadata (registers, spills, scratch,
LDS), the number of instructions and of MFMAs, and a hash of the instruction stream with comments, labels and directives
stripped and branch targets named by their block alone (not by the function's ordinal in its file).  The 256-VGPR kernels sit on a register-allocation knife edge (profiles/LABBOOK.md): a source change that is
meant to be neutral is checked by comparing two such listings before any GPU time is spent.

usage: kernel_resources.py [--csrc DIR] [--jobs N] [fdnn_chain.hip ...] > listing.txt
       kernel_resources.py --compare before.txt after.txt   (exit 1 if a kernel's resources grew or its MFMA count changed)"""
import argparse, concurrent.futures, glob, hashlib, os, re, shlex, subprocess, sys, tempfile

FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")
NOT_ABOVE = ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def compile_line(csrc, name):
    """The Makefile's compile command of NAME.hip, as a token list ending in the object file."""
    out = subprocess.run(["make", "-n", "-B", "-C", csrc, "../lib/%s.o" % name], capture_output=True, text=True, check=True).stdout
    for line in out.splitlines():
        tok = shlex.split(line, comments=True)
        if "-c" in tok and name + ".hip" in tok and "--cuda-device-only" not in tok:
            return tok
    raise SystemExit("no compile command for %s.hip in `make -n`" % name)


def to_assembly(csrc, name, tmp):
    tok = compile_line(csrc, name)
    flags = [t for t in tok[1:tok.index("-c")]]
    asm = os.path.join(tmp, name + ".s")
    subprocess.run([tok[0]] + flags + ["--cuda-device-only", "-S", name + ".hip", "-o", asm], cwd=csrc, check=True)
    return flags, asm


def kernels_of(asm):
    """-> {mangled name: dict of FIELDS + insts, mfma, hash}"""
    meta, cur, body, bodies = {}, None, None, {}
    for line in open(asm):
        m = re.match(r"  - \.(\w+):\s*(.*)", line)
        if m:  # a new entry of amdhsa.kernels
            cur = {}
            meta[id(cur)] = cur
        else:
            m = re.match(r"    \.(\w+):\s*(.*)", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2).strip().strip("'\"")
            continue
        t = line.split(";")[0].split("//")[0].strip()
        m = re.match(r"\.type\s+(\S+),@function", t)
        if m:
            body = bodies.setdefault(m.group(1), [])
        elif t.startswith(".Lfunc_end"):
            body = None
        elif body is not None and t and not t.startswith(".") and not t.endswith(":"):
            # (.LBB<function>_<block>: the function's ordinal in its file is no part of its code -- removing a kernel renumbers the rest)
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(t.split())))
    out = {}
    for k in meta.values():
        name = k.get("name")
        if name is None or name not in bodies:
            continue
        b = bodies[name]
        rec = {f: int(k.get(f, 0)) for f in FIELDS}
        rec["insts"] = len(b)
        rec["mfma"] = sum(1 for i in b if i.startswith("v_mfma"))
        rec["hash"] = hashlib.sha256("\n".join(b).encode()).hexdigest()[:16]
        out[name] = rec
    return out


def listing(csrc, jobs, only):
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(csrc, "*.hip")))
    names = [n for n in names if not only or n in only or n + ".hip" in only]
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        for name, (flags, asm) in zip(names, pool.map(lambda n: to_assembly(csrc, n, tmp), names)):
            print("# %s.hip: %s" % (name, " ".join(flags)))
            for kname, r in sorted(kernels_of(asm).items()):
                print("%s.hip %s %s insts=%d mfma=%d hash=%s" % (name, kname, " ".join("%s=%d" % (f, r[f]) for f in FIELDS), r["insts"], r["mfma"], r["hash"]))
            sys.stdout.flush()


def read_listing(path):
    out = {}
    for line in open(path):
        if line.startswith("#") or not line.strip():
            continue
        tok = line.split()
        out[(tok[0], tok[1])] = {k: (v if k == "hash" else int(v)) for k, v in (t.split("=") for t in tok[2:])}
    return out


def compare(before, after):
    a, b = read_listing(before), read_listing(after)
    bad = [("%s %s" % k, "only in " + (before if k in a else after)) for k in sorted(set(a) ^ set(b))]
    same = 0
    for k in sorted(set(a) & set(b)):
        x, y = a[k], b[k]
        if x["hash"] == y["hash"]:
            same += 1
            continue
        why = ["%s %d -> %d" % (f, x[f], y[f]) for f in NOT_ABOVE if y[f] > x[f]]
        if y["vgpr_count"] + y["agpr_count"] > x["vgpr_count"] + x["agpr_count"]:
            why.append("vgpr + agpr %d -> %d" % (x["vgpr_count"] + x["agpr_count"], y["vgpr_count"] + y["agpr_count"]))
        if x["mfma"] != y["mfma"]:
            why.append("mfma %d -> %d" % (x["mfma"], y["mfma"]))
        print("changed %s %s: insts %d -> %d (%+d), vgpr spills %d -> %d, sgpr spills %d -> %d, vgpr + agpr %d -> %d, sgpr %d -> %d%s"
              % (k[0], k[1], x["insts"], y["insts"], y["insts"] - x["insts"], x["vgpr_spill_count"], y["vgpr_spill_count"], x["sgpr_spill_count"],
                 y["sgpr_spill_count"], x["vgpr_count"] + x["agpr_count"], y["vgpr_count"] + y["agpr_count"], x["sgpr_count"], y["sgpr_count"],
                 "  ** " + "; ".join(why) if why else ""))
        if why:
            bad.append(("%s %s" % k, "; ".join(why)))
    print("%d kernels with the same instruction stream, %d changed, %d outside the conditions" % (same, len(set(a) & set(b)) - same, len(bad)))
    for name, why in bad:
        print("  %s: %s" % (name, why))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "fast-dnn_amd", "csrc"))
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--compare", nargs=2, metavar=("BEFORE", "AFTER"))
    ap.add_argument("files", nargs="*", help="translation units to list (default: every .hip of csrc)")
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else listing(args.csrc, args.jobs, args.files))
