#!/bin/bash
# Builds the HIP library for gfx950 in-tree (clarabel.jl_amd/), twice.  hipcc cross-compiles without a GPU.
#   libclarabel_hipkkt.so          the PRODUCT: what the Julia glue, bench.py and smoke() load.  Reads no HIPKKT_* switch (hipkkt_debug_set
#                                  refuses), contains neither the first form of the front-batch kernel nor the debug flags.
#   libclarabel_hipkkt_testing.so  the same sources with -DHIPKKT_TESTING + front_block.hip: what tests/ load (hipkkt_debug_set works).
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-result $HIPKKT_EXTRA_FLAGS"   # (development: e.g. -DHIPKKT_SWEEP_TRACE)
mkdir -p ../../build/obj ../../build/obj_testing
HOSTSRC="hipkkt_abi.cpp hipkkt_setup.cpp hipkkt_factor.cpp hipkkt_solve.cpp hipkkt_cones.cpp hipkkt_step.cpp symbolic.cpp solve_schedule.cpp ordering.cpp assemble.cpp"
# kernels are identical in both builds (nothing in a .hip file depends on HIPKKT_TESTING): compiled once
KSRC="kernels.hip values.hip solve_sweep.hip refine.hip assemble_dev.hip front_sweep.hip front_block2.hip probe.hip"
OBJ=../../build/obj
OBJT=../../build/obj_testing
pids=()
for f in $HOSTSRC; do
  $HIPCC $FLAGS -x c++ -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -c $f -o $OBJ/${f%.cpp}.o & pids+=($!)
done
# only the files that look at HIPKKT_TESTING are compiled a second time
for f in hipkkt_abi.cpp hipkkt_setup.cpp hipkkt_factor.cpp; do
  $HIPCC $FLAGS -DHIPKKT_TESTING -x c++ -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -c $f -o $OBJT/${f%.cpp}.o & pids+=($!)
done
for f in $KSRC; do
  $HIPCC $FLAGS -c $f -o $OBJ/${f%.hip}.o & pids+=($!)
done
$HIPCC $FLAGS -c front_block.hip -o $OBJT/front_block.o & pids+=($!)
# The cone kernels mirror the reference's formulas operation by operation, and the reference modules of tests/ emulate their rounding
# order: no FMA contraction.  scaling.hip, step.hip: the scaling and the step's cone algebra of the symmetric cones; step_cone3.hip,
# step_genpow.hip: the step of the Exponential / Power and the Generalized Power cones; step_psd.hip, step_psd_large.hip,
# scaling_psd.hip, scaling_psd_large.hip, barrier_psd.hip: step, Nesterov-Todd scaling and barrier of the PSD triangle cones (psd_cone.h); start.hip: the
# default start
KSRC_NOCONTRACT="scaling.hip step.hip step_cone3.hip step_genpow.hip step_psd.hip step_psd_large.hip scaling_psd.hip scaling_psd_large.hip start.hip barrier_psd.hip"
for f in $KSRC_NOCONTRACT; do
  $HIPCC $FLAGS -ffp-contract=off -c $f -o $OBJ/${f%.hip}.o & pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
COMMON="$OBJ/hipkkt_solve.o $OBJ/hipkkt_cones.o $OBJ/hipkkt_step.o $OBJ/symbolic.o $OBJ/solve_schedule.o $OBJ/ordering.o $OBJ/assemble.o $OBJ/assemble_dev.o $OBJ/scaling.o $OBJ/step.o $OBJ/step_cone3.o $OBJ/step_genpow.o $OBJ/step_psd.o $OBJ/step_psd_large.o $OBJ/scaling_psd.o $OBJ/scaling_psd_large.o $OBJ/start.o $OBJ/barrier_psd.o $OBJ/front_block2.o $OBJ/front_sweep.o $OBJ/probe.o $OBJ/kernels.o $OBJ/values.o $OBJ/solve_sweep.o $OBJ/refine.o"
$HIPCC --offload-arch=gfx950 -shared -fPIC -o ../libclarabel_hipkkt.so $OBJ/hipkkt_abi.o $OBJ/hipkkt_setup.o $OBJ/hipkkt_factor.o $COMMON
$HIPCC --offload-arch=gfx950 -shared -fPIC -o ../libclarabel_hipkkt_testing.so $OBJT/hipkkt_abi.o $OBJT/hipkkt_setup.o $OBJT/hipkkt_factor.o $OBJT/front_block.o $COMMON
echo "built $(readlink -f ../libclarabel_hipkkt.so) and $(readlink -f ../libclarabel_hipkkt_testing.so)"
