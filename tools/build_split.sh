#!/bin/bash
# The diagnostics library with the commit's check-step marks compiled in (-DKSCHED_COMMIT_SPLIT=1: trace columns 33-36 and 38-39,
# tools/trace_dist.py's "check step" lines), built from the working tree beside the plain library as
# k8s-scheduler_amd/libksched_split.so.  Select it with KSCHED_LIB and run under KSCHED_COMMIT_STAMPS=1
# KSCHED_PERSIST_TRACE=1 KSCHED_TRACE_DUMP=<file> (tools/gpu.sh trace).   bash tools/build_split.sh
set -e
cd "$(dirname "$0")/.."
make -s -j8 -C k8s-scheduler_amd BUILD=build_split LIB=libksched_split.so EXTRA=-DKSCHED_COMMIT_SPLIT=1
echo "built k8s-scheduler_amd/libksched_split.so"
