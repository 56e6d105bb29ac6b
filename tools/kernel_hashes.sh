#!/bin/bash
# "This edit changed no kernel": one line per gfx950 kernel of the library, no GPU needed --
#   symbol  sha256(instruction stream)  vgpr  sgpr  lds  scratch
# sorted by symbol, so that two listings diff cleanly when kernels move between translation units.  The hash covers
# the disassembly of the kernel's symbol without addresses and comments (local label numbers and the per-unit
# __hip_cuid symbol never enter it, nor does the alignment fill behind the code); the four numbers are the kernel descriptor's.
# usage: tools/kernel_hashes.sh [-C csrc-dir] [-u "unit ..."] [-- extra hipcc flags, e.g. -DBSR_BUCKET_MAX_PER_TILE=0]
#   tools/kernel_hashes.sh > new.txt; tools/kernel_hashes.sh -C build/base/bloomscene_amd/csrc > base.txt; diff base.txt new.txt
set -e
DIR="$(dirname "$0")/../bloomscene_amd/csrc"; UNITS=
while getopts "C:u:" o; do case $o in C) DIR=$OPTARG ;; u) UNITS=$OPTARG ;; *) exit 2 ;; esac; done
shift $((OPTIND - 1))
cd "$DIR"
[ -n "$UNITS" ] || UNITS=$(ls *.hip | sed 's/\.hip$//')
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}; LLVM=$(dirname "$($HIPCC --print-prog-name=clang)")
FLAGS=$(make -s print-FLAGS 2>/dev/null) || FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -mllvm -amdgpu-atomic-optimizer-strategy=None"
TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT
for u in $UNITS; do
	$HIPCC $FLAGS -fno-slp-vectorize "$@" --cuda-device-only --no-gpu-bundle-output -c $u.hip -o $TMP/$u.elf
	"$LLVM/llvm-objdump" -d --no-show-raw-insn $TMP/$u.elf > $TMP/$u.dis
	"$LLVM/llvm-readelf" --notes $TMP/$u.elf > $TMP/$u.notes
done
python3 - "$TMP" $UNITS <<'PY' | sort
import hashlib, re, sys
tmp, units = sys.argv[1], sys.argv[2:]
for u in units:
    desc = {}
    for blk in open(f"{tmp}/{u}.notes").read().split("  - .agpr_count:")[1:]:
        f = lambda key: re.search(rf"\.{key}:\s+(\S+)", blk).group(1)
        desc[f("name")] = (f("vgpr_count"), f("sgpr_count"), f("group_segment_fixed_size"), f("private_segment_fixed_size"))
    body = {}
    cur = None
    for line in open(f"{tmp}/{u}.dis"):
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = body.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(re.sub(r"\s*//.*$", "", line.strip()))
    for name, d in desc.items():
        while body[name] and body[name][-1] in ("s_nop 0", "..."):   # alignment fill behind the code (longest behind a unit's last kernel)
            body[name].pop()
        h = hashlib.sha256("\n".join(body[name]).encode()).hexdigest()
        print(f"{name}  {h}  {d[0]}  {d[1]}  {d[2]}  {d[3]}")
PY
