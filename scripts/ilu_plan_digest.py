"""The ILU(0) host analysis' digest lines (drivers/an_host_check.cpp: per
surrogate, a hash of the U plan and the digest of the whole plan) over the
surrogates the ILU host tests use, under each plan-time knob setting, one at a
time against the default. No GPU. profiles/r10_ilu_plan_digest.txt is its
output; a change to the analysis that is meant to keep the plans must
reproduce it.

    python scripts/ilu_plan_digest.py > lines.txt
        runs respasol_amd/build/asan/an_host_check_asan (make asan-an)
    python scripts/ilu_plan_digest.py --exe <an_host_check> > lines.txt
        runs another build of the same program (an optimised one takes a
        minute where the sanitizer build takes ten; an older tree's, with the
        U hash added to its an_host_check.cpp)
"""
import argparse
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "respasol_amd", "build", "asan", "an_host_check_asan")
SURROGATES = [("dc1", 0.3), ("G2_circuit", 0.05), ("ASIC_320ks", 0.1), ("ecology2", 0.05), ("parabolic_fem", 0.3),
              ("tmt_unsym", 0.05), ("FEM_3D_thermal2", 0.05)]
KNOBS = [{}] + [{k: v} for k, v in [
    ("RSP_ILU_SPLIT", "1"), ("RSP_ILU_GROUP", "2"), ("RSP_ILU_GROUP", "4"), ("RSP_ILU_THIN_SOLVE", "0"),
    ("RSP_ILU_THIN_TERMS", "256"), ("RSP_ILU_FAT_LONG", "0"), ("RSP_ILU_HUB", "64"), ("RSP_ILU_FAT_PAD", "0"),
    ("RSP_ILU_FLOW_PLAN", "0"), ("RSP_ILU_FLOW_GATE", "0"), ("RSP_ILU_THIN_FACTOR", "0"),
    ("RSP_ILU_THIN_FACTOR_ITEMS", "1024"), ("RSP_ILU_PIECE_ITEMS", "500"), ("RSP_ILU_FAC_ONE", "0"),
    ("RSP_ILU_FAC_SCALE", "0"), ("RSP_ILU_SLOT_PAD", "16"), ("RSP_ILU_PACK_PAIRS", "0"), ("RSP_ILU_BLOCKS", "0"),
    ("RSP_ILU_BLOCKS", "1"), ("OMP_NUM_THREADS", "1"), ("OMP_NUM_THREADS", "3"), ("OMP_NUM_THREADS", "8")]]
# a second knob on top of a first (a stored lower triangle plans one factor
# level: its pieces show only with RSP_ILU_FAC_ONE=0)
KNOBS.append({"RSP_ILU_FAC_ONE": "0", "RSP_ILU_PIECE_ITEMS": "500"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exe")
    args = ap.parse_args()
    if not args.exe:
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "respasol_amd", "csrc"), "asan-an"], check=True)
    base = {k: v for k, v in os.environ.items() if not k.startswith("RSP_")}
    base.update(OMP_NUM_THREADS="4", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for name, scale in SURROGATES:
        for knobs in KNOBS:
            tag = ",".join(f"{k}={v}" for k, v in knobs.items()) or "knobs-default"
            p = subprocess.run([args.exe or EXE, name, str(scale)], env=dict(base, **knobs), check=True,
                               capture_output=True, text=True)
            print(f"{tag:34s} {name}@{scale} {p.stdout.strip()}", flush=True)


if __name__ == "__main__":
    main()
