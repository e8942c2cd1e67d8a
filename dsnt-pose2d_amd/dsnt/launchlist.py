"""A recorded list of C-ABI launches and its replay.  It knows nothing of activations, convolutions or BatchNorm: it converts a
launch's arguments, keeps what they point to alive, counts the bytes its entries name, and replays itself — from C, one call per
segment, or entry by entry under a probe — on the streams of the `Lanes` it shares with its sibling list."""
import contextlib
import ctypes as C

import torch

from . import _lib


def check(lib, rc, name):
    if rc != 0:
        raise RuntimeError('%s failed (%d): %s' % (name, rc, lib.dsnt_last_error().decode()))


class Lanes:
    """The lanes of a tape's lists: 0 = the caller's stream, 1.. = side streams created at the first replay."""

    def __init__(self, use, n):
        self.use, self.n = use, n
        self.side = None

    def streams(self):
        main = torch.cuda.current_stream()
        if not self.use:
            return (main, None, None)
        if self.side is None:
            # (stream priorities were tried — chain on high-priority streams, weight gradients on a normal one — and
            # change nothing on this hardware)
            self.side = tuple(torch.cuda.Stream() for _ in range(self.n - 1))
        return (main,) + self.side


class LaunchList(list):
    """Entries (cfunc, converted args, name, lane); cfunc None: ('sync', (src, dst, event)) or ('bucket', k).

    keep: where structs are kept alive — the owner's list, or one of its own."""

    def __init__(self, lib, lanes, keep=None):
        super().__init__()
        self.lib, self.lanes = lib, lanes
        self.keep = [] if keep is None else keep
        self.nbytes, self.bytes_by_name = 0, {}
        self.workspace = set()      # data pointers of tensors that are workspace, not algorithm: left out of the byte counts
        self._into = self           # where new entries go (`into`)
        self._compiled = None

    @contextlib.contextmanager
    def into(self, lst):
        """Entries emitted inside the block go to `lst` (spliced in, or appended, later); they count as this list's."""
        saved, self._into = self._into, lst
        try:
            yield lst
        finally:
            self._into = saved

    def count(self, name, nb):
        self.nbytes += nb
        self.bytes_by_name[name] = self.bytes_by_name.get(name, 0) + nb

    def emit(self, lane, name, *args):
        fn = getattr(self.lib, name)
        conv = []
        for a in args:
            if isinstance(a, torch.Tensor):
                # algorithmic HBM bytes of the step (bench.py `step_bounds`): every tensor a launch names is read or
                # written once by it; weight-gradient slabs (workspace, not algorithm) are left out
                if a.data_ptr() not in self.workspace:
                    self.count(name, a.numel() * a.element_size())
                conv.append(_lib.ptr(a))
            elif isinstance(a, C.Structure):
                self.keep.append(a)
                conv.append(C.byref(a))
            else:
                conv.append(a)
        entry = (fn, tuple(conv), name, lane)
        self._into.append(entry)
        return entry

    @staticmethod
    def sync_entry(src, dst):
        """The entry at which `dst` lane waits for everything that stands before it on `src`."""
        return (None, (src, dst, torch.cuda.Event()), 'sync', 0)

    def sync(self, src, dst):
        self._into.append(self.sync_entry(src, dst))

    def mark(self, k, lane):
        """End of a segment: the replay calls its bucket hook with k, `lane`'s stream current."""
        self._into.append((None, k, 'bucket', lane))

    # ------------------------------------------------------------------ compiled form
    def record(self):
        """Record the entries into a fresh C launch list: (handle, (bucket, lane) after each segment).  The caller owns it."""
        lib, lanes = self.lib, self.lanes
        h = lib.dsnt_list_create()
        if not h:
            raise RuntimeError('dsnt_list_create failed')
        marks = []
        try:
            for lane in range(1, lanes.n) if lanes.use else ():
                check(lib, lib.dsnt_list_sync(h, 0, lane), 'dsnt_list_sync')
            check(lib, lib.dsnt_list_begin(h), 'dsnt_list_begin')
            try:
                for fn, args, name, lane in self:
                    if fn is not None:
                        check(lib, fn(*args, C.c_void_p(lane)), name)     # recorded, not launched: `stream` = lane index
                    elif name == 'sync':
                        check(lib, lib.dsnt_list_sync(h, args[0], args[1]), 'dsnt_list_sync')
                    else:
                        marks.append((args, lane))
                        lib.dsnt_list_mark(h)
            finally:
                lib.dsnt_list_end()
            for lane in range(1, lanes.n) if lanes.use else ():
                check(lib, lib.dsnt_list_sync(h, lane, 0), 'dsnt_list_sync')
        except Exception:
            lib.dsnt_list_destroy(h)
            raise
        return h, marks

    def compile(self):
        """(handle, marks) of the list as it stands at the first call; the list owns the handle."""
        if self._compiled is None:
            self._compiled = self.record()
        return self._compiled

    def __del__(self):
        try:
            if self._compiled is not None:
                self.lib.dsnt_list_destroy(self._compiled[0])
        except Exception:
            pass

    # ------------------------------------------------------------------ replay
    def replay(self, bucket_hook=None, probe=None):
        """Enqueue the list.  `probe(entry)` (diagnostics / tests) is called before every launch, which then go one by one."""
        lib, streams = self.lib, self.lanes.streams()
        main, sides = streams[0], streams[1:] if self.lanes.use else ()
        ptrs = tuple(st.cuda_stream if st is not None else 0 for st in streams)
        if probe is None:
            h, marks = self.compile()
            arr = (C.c_void_p * len(ptrs))(*ptrs)
            for seg in range(len(marks) + 1):
                self._check_launch(lib.dsnt_list_replay(h, seg, arr, len(ptrs)), 'dsnt_list_replay')
                if seg < len(marks) and bucket_hook is not None:
                    k, lane = marks[seg]
                    with torch.cuda.stream(streams[lane]):
                        bucket_hook(k)
            return
        for st in sides:
            st.wait_stream(main)
        for entry in self:
            fn, args, name, lane = entry
            if fn is not None:
                probe(entry)
                self._check_launch(fn(*args, ptrs[lane]), name)
            elif name == 'sync':
                src, dst, ev = args
                ev.record(streams[src])
                streams[dst].wait_event(ev)
            elif bucket_hook is not None:
                with torch.cuda.stream(streams[lane]):
                    bucket_hook(args)
        for st in sides:
            main.wait_stream(st)

    def _check_launch(self, rc, name):
        if rc != 0:
            torch.cuda.synchronize()
            check(self.lib, rc, name)
