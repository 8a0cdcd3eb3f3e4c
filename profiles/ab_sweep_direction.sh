#!/bin/bash
# A/B of the alternating tile sweep (sweep direction) on one box, in one call:
#   bash profiles/ab_sweep_direction.sh <checkout of the parent commit, built> [sets] [output directory]
# Per round: the parent build, this build, this build under BDG_SW2D_SWEEP=forward, one bench.py process each; three rounds per
# set, positions rotated in the even sets; then the smaller meshes and N = 8. One JSON line per run in
# <output directory>/sweep_ab.jsonl (default build/ab, which git ignores; profiles/r07_sweep_ab.jsonl holds the lines of round 7). Every run has its own time limit and the first failure ends the script.
set -eo pipefail
PARENT=$(cd "$1" && pwd)
SETS=${2:-3}
HERE=$(cd "$(dirname "$0")/.." && pwd)
OUTDIR=${3:-$HERE/build/ab}
mkdir -p "$OUTDIR"
OUT=$(cd "$OUTDIR" && pwd)/sweep_ab.jsonl
: > "$OUT"
run() { # build, tree, set, bench arguments, environment
    local build=$1 tree=$2 set=$3 args=$4 line
    shift 4
    line=$(cd "$tree" && env "$@" timeout -k 10 300 python bench.py --gpus 1 --no-cpu-baseline --no-also --steps 200 $args | tail -1)
    echo "{\"set\": \"$set\", \"build\": \"$build\", \"bench_args\": \"$args\", \"result\": $line}" >> "$OUT"
    echo "$set $build $args $(echo "$line" | python -c 'import json, sys; print(json.loads(sys.stdin.read())["ms_per_step"])')"
}
round() { # set, bench arguments, rotated
    if [ "$3" = 1 ]; then
        run default "$HERE" "$1" "$2" BDG_SW2D_SWEEP=
        run forward "$HERE" "$1" "$2" BDG_SW2D_SWEEP=forward
        run parent "$PARENT" "$1" "$2" BDG_SW2D_SWEEP=
    else
        run parent "$PARENT" "$1" "$2" BDG_SW2D_SWEEP=
        run default "$HERE" "$1" "$2" BDG_SW2D_SWEEP=
        run forward "$HERE" "$1" "$2" BDG_SW2D_SWEEP=forward
    fi
}
run parent "$PARENT" untimed "" BDG_SW2D_SWEEP=
run default "$HERE" untimed "" BDG_SW2D_SWEEP=
for set in $(seq 1 "$SETS"); do
    for r in 1 2 3; do round "head$set" "" $((1 - set % 2)); done
done
for cfg in "--cells 500x250" "--cells 700x360" "--order 8 --cells 500x250"; do
    for r in 1 2 3; do round other "$cfg" 0; done
done
