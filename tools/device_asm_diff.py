"""Does kai0_amd/csrc/NAME.hip in the work tree hold gfx950 device code that a revision does not?  A diff of two hipcc outputs, no GPU needed.
usage: python tools/device_asm_diff.py gemm_bf16 [--against REV]      (REV defaults to HEAD)
Both sides are compiled with build.py's flags plus --cuda-device-only -S; comment and directive lines (';' or '.' first) and blank lines are
dropped, and so is the __hip_cuid_ label, which differs between any two compiles.  The verdict: every function body of the work tree equals
the body of some function at REV — of the same name first, then of an unmatched one with the same instruction list (a rename: a dropped
template parameter changes the mangled name and nothing else).  Prints "identical"; or "no new device code" with the renamed pairs and REV's
functions that have no counterpart; or the work-tree functions whose body is new, and then exits 1."""
import re
import subprocess
import sys
import tempfile

name, rev = sys.argv[1], (sys.argv[sys.argv.index("--against") + 1] if "--against" in sys.argv else "HEAD")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", "-"]


def functions(asm):
    out, cur = {}, None
    for line in asm.split(".amdgpu_metadata")[0].splitlines():
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].strip())  # branch targets carry the function's position in the file
        if not line or line.startswith(".") or line.startswith("__hip_cuid_"):
            continue
        m = re.fullmatch(r"([A-Za-z_$][\w$.]*):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None:
            cur.append(line)
    return out


with tempfile.TemporaryDirectory() as tmp:
    subprocess.run(f"git archive {rev} kai0_amd/csrc include | tar -x -C {tmp}", shell=True, check=True)
    procs = [subprocess.Popen(["hipcc", *FLAGS, f"{root}/kai0_amd/csrc/{name}.hip"], stdout=subprocess.PIPE, text=True) for root in (tmp, ".")]
    old, new = (functions(p.communicate()[0]) for p in procs)
    if any(p.returncode for p in procs):
        sys.exit("hipcc failed")
if old == new:
    print("identical")
    sys.exit(0)
gone = [f for f in sorted(old) if old[f] != new.get(f)]  # REV's functions not matched by name
renamed, fresh = [], []
for f in sorted(new):
    if new[f] != old.get(f):
        twin = next((o for o in gone if old[o] == new[f]), None)
        if twin is None:
            fresh.append(f)
        else:
            gone.remove(twin)
            renamed.append((twin, f))
print(f"{len(fresh)} of {len(new)} function bodies are new ({rev} -> work tree):" if fresh else f"no new device code ({len(new) - len(renamed)} of {len(new)} functions unchanged)")
for f in fresh:
    print(f"  new      {f}  {len(new[f])} instructions")
for o, f in renamed:
    print(f"  renamed  {o} -> {f}  {len(new[f])} instructions")
for o in gone:
    if o not in new:  # (a function of the same name whose body changed is listed as new above)
        print(f"  removed  {o}  {len(old[o])} instructions")
sys.exit(1 if fresh else 0)
