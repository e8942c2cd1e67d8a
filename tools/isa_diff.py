"""Compare the device code of two builds of the library, function by function: python tools/isa_diff.py OLD.so NEW.so
[--rename OLD_SYMBOL=NEW_SYMBOL ...] (a kernel whose mangled name changed is compared under its new name).  Every gfx950 code object of each library is unbundled and disassembled; functions are keyed by symbol name across all code
objects (a kernel may move between translation units; a symbol that several objects hold is compared copy by copy).  A
function is identical when its instruction text (addresses and encodings dropped, cut at the symbol's size so that the padding
behind a function, zero fill included, does not count) and, for a kernel, its resource metadata agree.  Prints the identical,
changed, only-in-OLD and only-in-NEW lists; exit 1 if anything is changed or only in NEW."""
import glob, os, re, subprocess, sys, tempfile
LLVM = '/opt/rocm/lib/llvm/bin/'
META = ('vgpr_count', 'agpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size', 'max_flat_workgroup_size')


def _run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def functions(lib):
    """name -> sorted list of distinct (instruction text, metadata) copies over all gfx950 code objects of `lib`."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        tmp = os.path.join(d, 'lib.so')
        os.symlink(os.path.abspath(lib), tmp)
        _run(LLVM + 'llvm-objdump', '--offloading', tmp)
        for co in sorted(glob.glob(tmp + '.*gfx950')):
            end = {}                                    # symbol -> first address behind it
            for row in _run(LLVM + 'llvm-readelf', '-s', '--wide', co).split('\n'):
                f = row.split()
                if len(f) == 8 and f[3] == 'FUNC':
                    end[f[7]] = int(f[1], 16) + int(f[2])
            meta = {}
            for block in re.split(r'\n  - (?=\.)', _run(LLVM + 'llvm-readelf', '--notes', co)):
                kv = dict(re.findall(r'^    \.(\w+): +(\S+)', '    ' + block, re.M))     # (the kernel's own keys: four spaces deep)
                if 'name' in kv:
                    meta[kv['name']] = ' '.join('%s=%s' % (k, kv.get(k)) for k in META)
            name, body = None, []
            def close():
                if name is not None:
                    out.setdefault(name, set()).add(('\n'.join(body), meta.get(name, '')))
            for line in _run(LLVM + 'llvm-objdump', '-d', '--no-show-raw-insn', '--no-leading-addr', '--disassemble-zeroes', co).split('\n'):
                m = re.match(r'^<(.*)>:$', line)
                if m:
                    close()
                    name, body = m.group(1), []
                elif name is not None and line.strip():
                    text, _, note = line.partition('//')
                    addr = re.match(r'\s*([0-9A-Fa-f]+):', note)
                    if addr and name in end and int(addr.group(1), 16) >= end[name]:
                        continue                        # behind the symbol: alignment padding
                    body.append(text.strip())
            close()
    return {k: sorted(v) for k, v in out.items()}


def first_difference(a, b):
    for (ta, ma), (tb, mb) in zip(a, b):
        if ma != mb:
            return 'metadata: %s | %s' % (ma, mb)
        la, lb = ta.split('\n'), tb.split('\n')
        for i in range(max(len(la), len(lb))):
            x, y = (la[i] if i < len(la) else '<end>'), (lb[i] if i < len(lb) else '<end>')
            if x != y:
                return 'line %d: %s | %s' % (i + 1, x, y)
    return '%d copies | %d copies' % (len(a), len(b))


if __name__ == '__main__':
    args = sys.argv[1:]
    renames = {}                                        # --rename OLD=NEW (mangled names): compare OLD's function with NEW's
    while '--rename' in args:
        i = args.index('--rename')
        o, n = args[i + 1].split('=')
        renames[o] = n
        del args[i:i + 2]
    old, new = functions(args[0]), functions(args[1])
    old = {renames.get(k, k): v for k, v in old.items()}
    both = sorted(set(old) & set(new))
    same = [n for n in both if old[n] == new[n]]
    changed = [n for n in both if old[n] != new[n]]
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    for title, names in (('identical', same), ('changed', changed), ('only in OLD', only_old), ('only in NEW', only_new)):
        print('%s: %d' % (title, len(names)))
        for n in names:
            print('   ', n, ('  [' + first_difference(old[n], new[n]) + ']') if title == 'changed' else '')
    sys.exit(1 if changed or only_new else 0)
