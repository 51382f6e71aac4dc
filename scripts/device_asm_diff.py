"""Which device functions of a unit changed between two source states?  Compiles the unit's gfx950 assembly for a git revision (default HEAD,
via `git stash`-free `git show` into a temp tree) and for the working tree, strips comments / directives and compares function by function:
    python scripts/device_asm_diff.py [unit.hip] [rev]
Used in round 5 to show that a change to relmc_finalize_kernel left all 14 relmc_eval_kernel instantiations byte-identical.
A defaulted template argument that one side lacks (relmc_eval_kernel's ShapeDynamic) is dropped from the mangled names, so such an instantiation
is compared with its predecessor and not listed as one function gone and one new.  The HL1 kernels that were renamed or became instantiations
of a template (RENAMED) are compared with their predecessors in the same way."""
import hashlib, os, re, shutil, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "powersystemsreliabilityassessment_amd", "csrc")
unit = sys.argv[1] if len(sys.argv) > 1 else "relmc_core.hip"
rev = sys.argv[2] if len(sys.argv) > 2 else "HEAD"
AREA_ARGS = "PKNS_8AreaCaseEPKNS_8AreaTiesEPKdmmiiiilPd"
AREA_PACK = "PKNS_8AreaCaseEPKNS_8AreaTiesEPKdmmiiiilDpKT0_Pd"      # relmc_hl1_area_kernel<TIES, VAR...>: VAR empty, or AreaVarArgs for the former relmc_hl1_area_var_kernel<TIES>
RENAMED = {"_ZN5relmc21relmc_hl1_area_kernelEPKNS_8AreaCaseEPKdmmiiiilPd": "_ZN5relmc21relmc_hl1_area_kernelILb0EJEEEv" + AREA_PACK,
           "_ZN5relmc25relmc_hl1_area_tie_kernelE" + AREA_ARGS: "_ZN5relmc21relmc_hl1_area_kernelILb1EJEEEv" + AREA_PACK,
           "_ZN5relmc27relmc_hl1_seq_reduce_kernelEPKdlPd": "_ZN5relmc23relmc_hl1_reduce_kernelEPKdlPd"}
for ties in "01":
    RENAMED["_ZN5relmc21relmc_hl1_area_kernelILb%sEEEv" % ties + AREA_ARGS] = "_ZN5relmc21relmc_hl1_area_kernelILb%sEJEEEv" % ties + AREA_PACK
    RENAMED["_ZN5relmc25relmc_hl1_area_var_kernelILb%sEEEv" % ties + AREA_ARGS[:-2] + "NS_11AreaVarArgsEPd"] = "_ZN5relmc21relmc_hl1_area_kernelILb%sEJNS_11AreaVarArgsEEEEv" % ties + AREA_PACK
TRACK_ARGS = "PKNS_10Hl1SeqCaseEPKdmmliiNS_%sEPd"            # relmc_hl1_storage_track_kernel<0 | 1 | 2>: the storage, weather and stress kernels
for track, (was, args) in enumerate((("24relmc_hl1_storage_kernel", "14Hl1StorageArgs"), ("20relmc_hl1_var_kernel", "10Hl1VarArgs"), ("23relmc_hl1_stress_kernel", "13Hl1StressArgs"))):
    RENAMED["_ZN5relmc" + was + "E" + TRACK_ARGS % args] = "_ZN5relmc30relmc_hl1_storage_track_kernelILi%dEEEv" % track + TRACK_ARGS % "12Hl1TrackArgsIXT_EE4type"
CHAIN = "_ZN5relmc22relmc_hl1_chain_kernelILi%dELi%dEJ%sEEEvPKNS_10Hl1SeqCaseEPKdmmliiDpT1_"      # relmc_hl1_chain_kernel<MODEL, P, ARG...>: the sequential, event, sweep and maintenance kernels
RENAMED["_ZN5relmc20relmc_hl1_seq_kernelEPKNS_10Hl1SeqCaseEPKdmmliiPd"] = CHAIN % (0, 0, "rPd")
for p in (0, 1):
    RENAMED["_ZN5relmc22relmc_hl1_event_kernelILb%dEEEvPKNS_10Hl1SeqCaseEPKdmmliiiPyPNS_11Hl1EventRecEPxPKxllP15relmc_hl1_event" % p] = CHAIN % (1, p, "irPyrPNS_11Hl1EventRecErPxrPKxllrP15relmc_hl1_event")
for p in (1, 4, 8, 16):
    RENAMED["_ZN5relmc22relmc_hl1_sweep_kernelILi%dEEEvPKNS_10Hl1SeqCaseEPKdmmliiNS_12Hl1SweepArgsEPd" % p] = CHAIN % (2, p, "KNS_12Hl1SweepArgsErPd")
for p in (1, 2, 4, 8):                                       # the maintenance kernel, a template of its own at first, is the template's fourth model
    RENAMED["_ZN5relmc22relmc_hl1_maint_kernelILi%dEEEvPKNS_10Hl1SeqCaseEPKdmmliiddiPKjPd" % p] = CHAIN % (3, p, "ddirPKjrPd")


def asm(csrc, out):
    if not os.path.exists(os.path.join(csrc, unit)):          # a unit that one side does not have yet (or any more): no device functions there
        open(out, "w").close(); return
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", out, os.path.join(csrc, unit)],
                          stderr=subprocess.DEVNULL)


def funcs(path):
    out, cur, buf = {}, None, []
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur, buf = m.group(1).replace("NS_12ShapeDynamicE", ""), []
            cur = RENAMED.get(cur, cur)
        elif cur is not None:
            if ln.startswith(".Lfunc_end"):
                out[cur] = buf; cur = None
            elif not ln.strip().startswith((";", ".")):
                buf.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r";.*", "", ln)).strip())      # block labels carry the function's ordinal in the unit
    return out


with tempfile.TemporaryDirectory() as tmp:
    old = os.path.join(tmp, "old"); os.makedirs(os.path.join(old, "powersystemsreliabilityassessment_amd"))
    subprocess.check_call(f"git -C {ROOT} archive {rev} powersystemsreliabilityassessment_amd/csrc include | tar -x -C {old}", shell=True)
    asm(os.path.join(old, "powersystemsreliabilityassessment_amd", "csrc"), os.path.join(tmp, "old.s"))
    asm(CSRC, os.path.join(tmp, "new.s"))
    a, b = funcs(os.path.join(tmp, "old.s")), funcs(os.path.join(tmp, "new.s"))
    sub = lambda n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip()[:110]
    for k in sorted(set(a) | set(b)):
        same = hashlib.sha256("\n".join(a.get(k, [])).encode()).digest() == hashlib.sha256("\n".join(b.get(k, [])).encode()).digest()
        print(("same " if same else "DIFF ") + sub(k), len(a.get(k, [])), "->", len(b.get(k, [])), "instructions")
    print(f"{unit}: {len(set(a) | set(b))} device functions, {sum(a.get(k) != b.get(k) for k in set(a) | set(b))} differ")
