#!/bin/bash
# indep_time.py under several library builds, alternating (diagnostics): LIBS, REPS.
# Two libraries are timed in ONE process (A B A B ..., REPS rounds, default 5);
# any other number runs one process per library and round.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/../..}"
set -- ${LIBS}
if [ $# -eq 2 ]; then
  timeout -k 10 300 python -u scripts/dev/indep_time.py "$PWD/$1" "$PWD/$2" "${REPS:-5}" 2>&1 | grep -v amdgpu.ids
  exit "${PIPESTATUS[0]}"
fi
for i in $(seq ${REPS:-2}); do
  for L in ${LIBS}; do
    XCGPU_LIB=$PWD/$L timeout -k 10 120 python -u scripts/dev/indep_time.py 2>&1 | grep -v amdgpu.ids || exit 1
  done
done
