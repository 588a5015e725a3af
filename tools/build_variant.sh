#!/bin/bash
# tools/build_variant.sh NAME [-DFLAG ...]: an A/B build of the library into build_ab/libgaml_hip_NAME.so (load it with
# GAML_HIP_LIB=...), with the register / scratch use of the paired scoring kernels (the multi-set kernel's and the coverage
# sweeps' and the gap profile's table kernel and the PacBio and single-end scorers and the PacBio coverage sweeps (the block-per-contig pacbio_path_sweep_kernel among them) and the single-end table build's kernels with LDS and scalar registers) and of the aligner's span and extension kernels (both instantiations) printed: a variant that spills to scratch is not worth a GPU run.
set -e
NAME=$1; shift
HERE=$(cd "$(dirname "$0")/.." && pwd)
SRC=$HERE/gaml_amd/csrc
T=/tmp/gaml_variant_$NAME; mkdir -p $T $HERE/build_ab
FL="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-function -Wno-sign-compare"
# (variants are development builds: the probes that load them use knobs and debug entry points)
(cd $SRC && /opt/rocm/bin/hipcc $FL -DGAML_HIP_DEV "$@" -Rpass-analysis=kernel-resource-usage -c gaml_hip.hip -o $T/gaml_hip.o > $T/usage.txt 2>&1) || { tail -20 $T/usage.txt; exit 1; }
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $HERE/build_ab/libgaml_hip_$NAME.so $SRC/obj_dev/host_model.o $T/gaml_hip.o $SRC/obj_dev/multi.o $SRC/obj_dev/version.o -ldl -lpthread
python3 - $T/usage.txt $NAME <<'PY'
import re, sys
t = open(sys.argv[1]).read()
for b in re.split(r"remark: Function Name: ", t)[1:]:
    name = b.split()[0]
    g = lambda k: (re.search(k + r": (\d+)", b) or [None, "?"])[1]
    aln = re.search(r"(span_maxima_kernel|span_cands_kernel|extend_kernel|extend_pair2_kernel)ILi(\d+)E", name)  # the aligner's instantiations (aligner.hip.h)
    if aln: print(sys.argv[2], f"{aln.group(1)}<{aln.group(2)}>", "VGPR", g("VGPRs"), "SGPR", g("SGPRs"), "LDS", g(r"LDS Size \[bytes/block\]"), "scratch", g(r"ScratchSize \[bytes/lane\]"), "spillV", g("VGPRs Spill"), "spillS", g("SGPRs Spill"), "waves/SIMD", g(r"Occupancy \[waves/SIMD\]"))
    # the multi-set scoring kernel (template arguments: GEN, COV) and the coverage sweeps: LDS and scalar registers too
    if "paired_score_multi_kernel" in name or "coverage_sweep" in name or "gap_tables_kernel" in name or "pacbio_score" in name or "pacbio_path_sweep" in name or "pacbio_sweep_kernel" in name or "single_score" in name or re.search(r"st_(clear|keys|heads|fill)_kernel", name):
        print(sys.argv[2], name, "VGPR", g("VGPRs"), "SGPR", g("SGPRs"), "LDS", g(r"LDS Size \[bytes/block\]"), "scratch", g(r"ScratchSize \[bytes/lane\]"), "spillV", g("VGPRs Spill"), "spillS", g("SGPRs Spill"), "waves/SIMD", g(r"Occupancy \[waves/SIMD\]"))
    if "paired_score_kernel" not in name: continue
    print(sys.argv[2], name[22:60], "VGPR", g("VGPRs"), "scratch", g(r"ScratchSize \[bytes/lane\]"), "spillV", g("VGPRs Spill"), "spillS", g("SGPRs Spill"))
PY
