"""d_exp_half_neg (gridpp_amd/csrc/oi_common.h): exp(-v^2 / 2) from t = v^2 with the factor -1/2 folded into the constants of the table
exp.  The CPU restatement of both forms (tools/ubench/exp_half_sq.c) must return the very double of d_exp_core(-0.5 v v) for every 64th
float32 v in [0, 15], for v = 0, v = 15, the smallest normal and subnormal v."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constants(body):
    return re.findall(r"[-+]?\d\.\d+e[-+]\d+(?: / [\d.]+)?|-?184\.\d+(?: / 2\.0)?|0\.125|-0\.5\b", body)


def test_restatement_has_the_constants_of_the_kernel():
    """(the C file is only evidence for the kernel if it states the same arithmetic: the constants of the two d_exp_half_neg bodies, in order)"""
    hdr = open(os.path.join(ROOT, "gridpp_amd", "csrc", "oi_common.h")).read()
    csrc = open(os.path.join(ROOT, "tools", "ubench", "exp_half_sq.c")).read()
    dev = hdr[hdr.index("double d_exp_half_neg(double t) {"):]
    dev = dev[:dev.index("ldexp")]
    cpu = csrc[csrc.index("double e_half_neg(double t){"):]
    cpu = cpu[:cpu.index("ldexp")]
    assert len(_constants(dev)) == 8 and _constants(dev) == _constants(cpu), (_constants(dev), _constants(cpu))


def test_rescaled_exponential_returns_the_same_double(tmp_path):
    exe = str(tmp_path / "exp_half_sq")
    ub = os.path.join(ROOT, "tools", "ubench")
    # (explicit fma() calls, no contraction of anything else; with the hardware instruction where the machine has one -- the library routine gives the same values, slower)
    flags = ["-O2", "-ffp-contract=off"]
    try:
        if " fma " in open("/proc/cpuinfo").read():
            flags.append("-mfma")
    except OSError:
        pass
    subprocess.run(["gcc"] + flags + ["-o", exe, os.path.join(ub, "exp_half_sq.c"), "-lm"], check=True, cwd=ub)
    r = subprocess.run([exe, "64"], capture_output=True, text=True)
    m = re.search(r"n=(\d+) mismatches (\d+)", r.stdout)
    assert m, r.stdout + r.stderr
    assert int(m.group(1)) > 17000000 and int(m.group(2)) == 0 and r.returncode == 0, r.stdout
