"""Compare the gfx950 ISA of two builds of the library, function by function.

    hipcc -O3 --offload-arch=gfx950 -std=c++17 --cuda-device-only -S -o a.s <tree A>/zero-inflated-gp_amd/csrc/zigp_lib.hip
    hipcc ...                                                        -o b.s <tree B>/zero-inflated-gp_amd/csrc/zigp_lib.hip
    python tools/isa_compare.py a.s b.s > profiles/<name>_isa.log

A cross-compile is enough: no GPU is needed.  A function's body is its lines between `name:` and `.Lfunc_end`, with comment-only lines
and the `; ...` tails dropped; local labels carry the function's number in the file and are renumbered by first appearance, so a function
that only moved in the file compares equal.  Exit status 1 when a function of A is missing from B or differs."""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r'^(_Z\w+|\w+):\s*(;.*)?$', line)
        if name is None:
            if m and not line.startswith('.'):
                name, body = m.group(1), []
            continue
        if line.startswith('.Lfunc_end'):
            out[name] = renumber(body)
            name = None
            continue
        code = line.split(';')[0].rstrip()
        if code.strip():
            body.append(code)
    return out


def renumber(body):
    seen = {}

    def sub(m):
        return seen.setdefault(m.group(0), '.L%d' % len(seen))
    return [re.sub(r'\.L[A-Za-z_]*\d+(_\d+)?', sub, ln) for ln in body]


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    same = [k for k in a if k in b and a[k] == b[k]]
    diff = [k for k in a if k in b and a[k] != b[k]]
    gone = [k for k in a if k not in b]
    new = [k for k in b if k not in a]
    print('functions in A: %d, in B: %d' % (len(a), len(b)))
    print('identical: %d   different: %d   only in A: %d   only in B: %d' % (len(same), len(diff), len(gone), len(new)))
    for k in diff:
        print('DIFFERENT  %s  (%d vs %d instructions)' % (k, len(a[k]), len(b[k])))
    for k in gone:
        print('ONLY IN A  %s' % k)
    for k in new:
        print('only in B  %s  (%d lines)' % (k, len(b[k])))
    return 1 if diff or gone else 0


if __name__ == '__main__':
    sys.exit(main())
