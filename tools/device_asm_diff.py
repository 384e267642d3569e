"""Is the gfx950 device code of kai0_amd/csrc/NAME.hip the same in the work tree as at a revision?  A diff of two hipcc outputs, no GPU needed.
usage: python tools/device_asm_diff.py gemm_bf16 [--against REV]      (REV defaults to HEAD)
Both sides are compiled with build.py's flags plus --cuda-device-only -S; comment and directive lines (';' or '.' first) and blank lines are
dropped, and so is the __hip_cuid_ label, which differs between any two compiles.  Prints "identical", or the functions whose bodies differ."""
import re
import subprocess
import sys
import tempfile

name, rev = sys.argv[1], (sys.argv[sys.argv.index("--against") + 1] if "--against" in sys.argv else "HEAD")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", "-"]


def functions(asm):
    out, cur = {}, None
    for line in asm.split(".amdgpu_metadata")[0].splitlines():
        line = line.split(";")[0].strip()
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
differ = [f for f in sorted(set(old) | set(new)) if old.get(f) != new.get(f)]
print("identical" if not differ else f"{len(differ)} of {len(new)} function bodies differ ({rev} -> work tree instructions):")
for f in differ:
    print(f"  {f}  {len(old.get(f, []))} -> {len(new.get(f, []))}")
sys.exit(1 if differ else 0)
