"""The reference's front-end answers, live or replayed.

tests/test_tokenizer.py and tests/test_audio_frontend.py compare the product with the REFERENCE's own tokenizer, WAV reader,
resampler and log-mel, compiled into oracle/_ref/libleaxer_ref.so by oracle/build_ref.py where the reference's sources are at
hand.  Where they are not, the same calls are answered from tests/golden/<function>_answers.npz: every call those tests make, keyed
by the bytes it passes (file contents, samples, text, and for the tokenizer the load history that set its process-global state),
with what the library returned.  `Q3TTS_RECORD_REF=1` with the library present rewrites those files from it."""
import ctypes as C
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FUNCS = ("ref_read_wav", "ref_resample", "ref_mel", "ref_tokenizer")


def _key(*parts):
    h = hashlib.sha1()
    for p in parts:
        p = p if isinstance(p, bytes) else repr(p).encode()
        h.update(len(p).to_bytes(8, "little") + p)
    return h.hexdigest()


def _file(path):
    try:
        with open(path, "rb") as f:
            return b"file:" + f.read()
    except OSError:
        return b"missing"


def _mem(ptr, nbytes):
    return C.string_at(ptr, nbytes) if ptr and nbytes > 0 else b""


class RefIO:
    """The library's C entry points (oracle/ref_shim/ref_io_shim.cpp) with the same arguments, over the live library when `so` exists,
    else over the recorded answers.  A call that was never recorded fails: the test then feeds the reference something new."""

    def __init__(self, so):
        self.L = None
        if so and os.path.exists(so):
            L = C.CDLL(so)
            L.ref_read_wav.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
            L.ref_resample.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
            L.ref_mel.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
            L.ref_tok_load.argtypes = [C.c_char_p, C.c_char_p]
            L.ref_tokenize.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int32), C.c_int]
            self.L = L
        self.recording = self.L is not None and os.environ.get("Q3TTS_RECORD_REF") == "1"
        self.ans = {f: {} for f in FUNCS}
        if self.L is None:
            for f in FUNCS:
                p = os.path.join(GOLDEN, f + "_answers.npz")
                if os.path.exists(p):
                    with np.load(p) as z:   # one row per call: key, its integer results, its slice of the concatenated values
                        keys, ints, offs, vals = z["keys"], z["ints"], z["offs"], z["vals"]
                    self.ans[f] = {k.decode(): (ints[i], vals[offs[i]:offs[i + 1]]) for i, k in enumerate(keys)}
        self.tok_state = "init"   # the reference's tokenizer is one process-global instance: what it holds follows the loads so far

    @property
    def live(self):
        return self.L is not None

    def _call(self, func, key, live_call):
        """live: run the library, keep (ints, values) when recording; replay: the recorded (ints, values)"""
        if self.live:
            ints, vals = live_call()
            if self.recording:
                self.ans[func][key] = (ints, vals)
            return ints, vals
        if key not in self.ans[func]:
            raise AssertionError(f"{func}: no recorded answer of the reference for this input (tests/golden/{func}_answers.npz; "
                                 "re-record with Q3TTS_RECORD_REF=1 where the reference's sources are present)")
        ints, vals = self.ans[func][key]
        return [int(x) for x in ints], vals

    def save(self):
        if not self.recording:
            return
        for f, a in self.ans.items():
            if a:
                keys = sorted(a)
                width = max(len(a[k][0]) for k in keys)
                ints = np.array([list(a[k][0]) + [0] * (width - len(a[k][0])) for k in keys], np.int64)
                offs = np.cumsum([0] + [len(a[k][1]) for k in keys]).astype(np.int64)
                vals = np.concatenate([a[k][1] for k in keys])
                np.savez_compressed(os.path.join(GOLDEN, f + "_answers.npz"), keys=np.array(keys, "S40"), ints=ints, offs=offs, vals=vals)

    # ---- audio ----
    def ref_read_wav(self, path, buf, cap, sr_ref):
        def live():
            out = np.zeros(cap, np.float32)
            sr = C.c_int(-1)
            n = self.L.ref_read_wav(path, out.ctypes.data, cap, C.byref(sr))
            return (n, sr.value), out[:max(0, min(n, cap))].copy()
        (n, sr), vals = self._call("ref_read_wav", _key(_file(path), cap), live)
        C.memmove(buf, np.ascontiguousarray(vals, np.float32).ctypes.data, 4 * len(vals))
        sr_ref._obj.value = sr
        return n

    def ref_resample(self, src_ptr, n, src, dst, out_ptr, cap):
        def live():
            out = np.zeros(cap, np.float32)
            m = self.L.ref_resample(src_ptr, n, src, dst, out.ctypes.data, cap)
            return (m,), out[:max(0, min(m, cap))].copy()
        (m,), vals = self._call("ref_resample", _key(_mem(src_ptr, 4 * n), n, src, dst, cap), live)
        C.memmove(out_ptr, np.ascontiguousarray(vals, np.float32).ctypes.data, 4 * len(vals))
        return m

    def ref_mel(self, src_ptr, n, out_ptr, cap):
        def live():
            out = np.zeros(max(cap, 0), np.float32)
            k = self.L.ref_mel(src_ptr, n, out.ctypes.data if cap > 0 else None, cap)
            return (k,), out[:max(0, min(k, cap))].copy()
        (k,), vals = self._call("ref_mel", _key(_mem(src_ptr, 4 * n), n, cap), live)
        if len(vals):
            C.memmove(out_ptr, np.ascontiguousarray(vals, np.float32).ctypes.data, 4 * len(vals))
        return k

    # ---- tokenizer ----
    def ref_tok_load(self, vocab, merges):
        files = _key(_file(vocab), _file(merges))
        (r,), _ = self._call("ref_tokenizer", _key("load", self.tok_state, files),
                             lambda: ((self.L.ref_tok_load(vocab, merges),), np.zeros(0, np.int32)))
        # both tables are cleared and re-read on every load: after a load that read both, what it holds is those two files
        self.tok_state = "loaded:" + files if r == 3 else _key(self.tok_state, files, r)
        return r

    def ref_tok_ready(self):
        (r,), _ = self._call("ref_tokenizer", _key("ready", self.tok_state), lambda: ((self.L.ref_tok_ready(),), np.zeros(0, np.int32)))
        return r

    def ref_tokenize(self, text, n, buf, cap):
        def live():
            out = (C.c_int32 * cap)()
            m = self.L.ref_tokenize(text, n, out, cap)
            return (m,), np.array(out[:max(0, min(m, cap))], np.int32)
        (m,), vals = self._call("ref_tokenizer", _key("tokenize", self.tok_state, text[:n], cap), live)
        for i, v in enumerate(vals):
            buf[i] = int(v)
        return m
