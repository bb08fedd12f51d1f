#!/usr/bin/env bash
# Is the device code of the working tree the same, instruction for instruction, as that of another revision?
#     tools/device_code_diff.sh <rev>
# Compiles the five translation units of the library to gfx950 assembly (device side only, the Makefile's flags, no DEFS) from the working
# tree and from <rev> (checked out into a temporary git worktree), replaces the compiler's hash of the source text (__hip_cuid_<hex>, the
# only difference a pure source move leaves) by a fixed token and compares.  One line per unit, `identical` or `DIFFERS`; the exit status
# is non-zero if any unit differs or fails to compile.  CPU only: nothing runs on a GPU.  Ten compilations, JOBS (default 5) at a time.
set -u
rev=${1:?usage: tools/device_code_diff.sh <rev>}
root=$(cd "$(dirname "$0")/.." && pwd)
hipcc=${HIPCC:-/opt/rocm/bin/hipcc}
jobs=${JOBS:-5}
units="ocean_api frames_small frames_mid frames_2048 frames_4096"
tmp=$(mktemp -d)
trap 'git -C "$root" worktree remove --force "$tmp/rev" >/dev/null 2>&1; rm -rf "$tmp"' EXIT
git -C "$root" worktree add --detach "$tmp/rev" "$rev" >/dev/null 2>&1 || { echo "cannot check out $rev" >&2; exit 2; }
mkdir -p "$tmp/a" "$tmp/b"
compile() {     # <source tree> <output directory> <unit>
    (cd "$1/watersurfacerendering_amd/csrc" &&
     "$hipcc" -O3 -std=c++17 -fPIC --offload-arch=gfx950 -S --cuda-device-only -o "$2/$3.raw" "$3.hip" 2> "$2/$3.log" &&
     sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$2/$3.raw" > "$2/$3.s")
}
export -f compile
export hipcc
for u in $units; do printf '%s\0%s\0%s\0' "$tmp/rev" "$tmp/a" "$u" "$root" "$tmp/b" "$u"; done |
    xargs -0 -n 3 -P "$jobs" bash -c 'compile "$@"' _
status=0
for u in $units; do
    if [ ! -s "$tmp/a/$u.s" ] || [ ! -s "$tmp/b/$u.s" ]; then
        echo "$u: DIFFERS (did not compile)"; cat "$tmp/a/$u.log" "$tmp/b/$u.log" >&2; status=1
    elif cmp -s "$tmp/a/$u.s" "$tmp/b/$u.s"; then
        echo "$u: identical ($(grep -c '^\s*\.amdhsa_kernel ' "$tmp/b/$u.s") kernels, $(wc -l < "$tmp/b/$u.s") lines)"
    else
        echo "$u: DIFFERS ($(diff "$tmp/a/$u.s" "$tmp/b/$u.s" | grep -c '^[<>]') lines)"; status=1
    fi
done
exit $status
