#!/bin/bash
# development: libasr variants for A/B timing and the trace builds (tools/blktrace.py, stacktrace.py, tracebench.py,
# stampbench.py).  usage: tools/build_variants.sh NAME "-DFLAG=.." [NAME "-D.."]...
# NAME=head builds the committed sources (git HEAD) instead of the working tree.  The sources are _build.SOURCES.
cd "$(dirname "$0")/.."
P=differential_equations_resnet_amd
S=$P/csrc
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  root=.
  if [ $name = head ]; then root=$(mktemp -d) && git archive HEAD $P/_build.py $S include | tar -x -C $root; fi
  srcs=$(cd $root/$P && python -c "import _build; print(' '.join('$root/$S/' + s for s in _build.SOURCES))")
  /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -shared $flags -o build_abl_$name.so $srcs &
done
wait
ls -la build_abl_*.so
