#!/bin/bash
# usage: tools/var_bench.sh "name1 name2 ..." [bench args]; logs go to $VAR_OUT (default var_out/)
export TMPDIR=/tmp
V=$1; shift
O=${VAR_OUT:-var_out}; mkdir -p $O
for v in base $V; do
  if [ "$v" = base ]; then unset MPCB_LIB; else export MPCB_LIB=$PWD/mpc_blaster_amd/variants/lib_$v.so; fi
  timeout -k 10 120 python bench.py --full --no-cpu-baseline "$@" > $O/var_$v.log 2>&1 || { echo "fail $v"; exit 1; }
done
