#!/usr/bin/env bash
# Is the device code of the working tree the same, instruction for instruction, as that of another revision -- wherever its functions live?
#     tools/device_code_diff.sh <rev>
# Compiles every csrc/*.hip each tree has to gfx950 assembly (device side only, the Makefile's flags, no DEFS), the working tree's and that of
# <rev> (checked out into a temporary git worktree), cuts each unit at the compiler's `; -- Begin function X` / `; -- End function` markers and
# compares PER FUNCTION SYMBOL ACROSS ALL UNITS: a kernel that moved from one unit to another is the same kernel.  Body and kernel descriptor
# are compared after replacing what depends on a function's position in its unit by fixed tokens: the N of the local labels .LBBN_ (of
# the BBN_ in loop comments too, and the padding between such a label and its comment, which its length decides), the N of .Lfunc_endN, and the compiler's hash of the unit's source text (__hip_cuid_<hex>).  A symbol that
# occurs in several units is compared per occurrence (same unit first, the rest in unit order).
# Output: one line per unit (kernels, functions, lines); one line for every symbol that differs, appeared or disappeared; one line per pair
# of units that symbols moved between.  The exit status is non-zero unless both trees have the same set of symbols, every one identical, and
# every unit compiled.  CPU only: nothing runs on a GPU.  JOBS (default 6) compilations at a time.
set -u
rev=${1:?usage: tools/device_code_diff.sh <rev>}
root=$(cd "$(dirname "$0")/.." && pwd)
hipcc=${HIPCC:-/opt/rocm/bin/hipcc}
jobs=${JOBS:-6}
tmp=$(mktemp -d)
trap 'git -C "$root" worktree remove --force "$tmp/rev" >/dev/null 2>&1; rm -rf "$tmp"' EXIT
git -C "$root" worktree add --detach "$tmp/rev" "$rev" >/dev/null 2>&1 || { echo "cannot check out $rev" >&2; exit 2; }
mkdir -p "$tmp/a" "$tmp/b"
compile() {     # <source tree> <output directory> <unit>
    (cd "$1/watersurfacerendering_amd/csrc" &&
     "$hipcc" -O3 -std=c++17 -fPIC --offload-arch=gfx950 -S --cuda-device-only -o "$2/$3.s" "$3.hip" 2> "$2/$3.log") || rm -f "$2/$3.s"
}
export -f compile
export hipcc
units_of() { (cd "$1/watersurfacerendering_amd/csrc" && ls *.hip | sed 's/\.hip$//'); }
{ for u in $(units_of "$tmp/rev"); do printf '%s\0%s\0%s\0' "$tmp/rev" "$tmp/a" "$u"; done
  for u in $(units_of "$root"); do printf '%s\0%s\0%s\0' "$root" "$tmp/b" "$u"; done; } |
    xargs -0 -n 3 -P "$jobs" bash -c 'compile "$@"' _
status=0
for f in "$tmp"/a/*.log "$tmp"/b/*.log; do
    if [ ! -s "${f%.log}.s" ]; then echo "$(basename "$f" .log): DIFFERS (did not compile)"; cat "$f" >&2; status=1; fi
done
python3 - "$tmp/a" "$tmp/b" "$rev" <<'EOF' || status=1
import collections, glob, os, re, subprocess, sys

POSITION = [(re.compile(r'__hip_cuid_[0-9a-f]+'), '__hip_cuid_X'), (re.compile(r'(\.L|\b)BB[0-9]+_'), r'\1BBN_'), (re.compile(r'\.Lfunc_end[0-9]+'), '.Lfunc_endN'),
            (re.compile(r'^(\.LBBN_[0-9]+:)\s+;'), r'\1 ;')]

def functions(tree):
    """{unit: (kernels, functions, lines)}, {symbol: [(unit, normalised text)]} of one tree's assembly."""
    stats, found = {}, collections.defaultdict(list)
    for path in sorted(glob.glob(os.path.join(tree, '*.s'))):
        unit, name, body, kernels, count = os.path.basename(path)[:-2], None, [], 0, 0
        lines = open(path).read().split('\n')
        for line in lines:
            begin = re.search(r'; -- Begin function (\S+)', line)
            if begin:
                name, body = begin.group(1), []
            if name is None:
                continue
            for pattern, token in POSITION:
                line = pattern.sub(token, line)
            body.append(line)
            if '; -- End function' in line:
                found[name].append((unit, '\n'.join(body)))
                kernels += any(l.lstrip().startswith('.amdhsa_kernel ') for l in body)
                count += 1
                name = None
        stats[unit] = (kernels, count, len(lines))
    return stats, found

def readable(symbols):
    try:
        out = subprocess.run(['c++filt'], input='\n'.join(symbols), capture_output=True, text=True, check=True).stdout.split('\n')
        return {s: re.sub(r'\(.*', '', d) for s, d in zip(symbols, out)}      # (without the parameter list)
    except (OSError, subprocess.CalledProcessError):
        return {s: s for s in symbols}

(stats_a, found_a), (stats_b, found_b) = functions(sys.argv[1]), functions(sys.argv[2])
describe = lambda s: '%d kernels, %d functions, %d lines' % s
for unit in sorted(set(stats_a) | set(stats_b)):
    a, b = stats_a.get(unit), stats_b.get(unit)
    print('%s: %s' % (unit, 'only in %s (%s)' % (sys.argv[3], describe(a)) if b is None else
                      describe(b) + ('' if a == b else ' (new unit)' if a is None else ' (%s: %s)' % (sys.argv[3], describe(a)))))
names = readable(sorted(set(found_a) | set(found_b)))
bad, moved = 0, collections.defaultdict(list)
for symbol in sorted(names):
    a, b = found_a.get(symbol, []), found_b.get(symbol, [])
    if len(a) != len(b):
        what = 'appeared in ' + ', '.join(u for u, _ in b) if not a else 'disappeared from ' + ', '.join(u for u, _ in a) if not b else \
               'DIFFERS: %d occurrences (%s), were %d (%s)' % (len(b), ', '.join(u for u, _ in b), len(a), ', '.join(u for u, _ in a))
        print('%s: %s' % (names[symbol], what))
        bad += 1
        continue
    same_unit = set(u for u, _ in a) & set(u for u, _ in b)       # pair the occurrences: same unit first, the rest in unit order
    order = lambda occurrences: sorted(occurrences, key=lambda o: (o[0] not in same_unit, o[0]))
    for (ua, ta), (ub, tb) in zip(order(a), order(b)):
        if ta != tb:
            la, lb = ta.split('\n'), tb.split('\n')
            print('%s: DIFFERS (%s -> %s: %d -> %d lines, %d differ)' % (names[symbol], ua, ub, len(la), len(lb),
                                                                        sum(x != y for x, y in zip(la, lb)) + abs(len(la) - len(lb))))
            bad += 1
        elif ua != ub:
            moved[(ua, ub)].append(names[symbol])
for (ua, ub), symbols in sorted(moved.items()):
    print('moved %s -> %s, identical: %s' % (ua, ub, ', '.join(symbols)))
total = sum(len(v) for v in found_b.values())
print('%d symbols, %s' % (total, 'all identical' if not bad else '%d differ, appeared or disappeared' % bad))
sys.exit(1 if bad or not total else 0)
EOF
exit $status
