"""G.711 on the host (include/q3tts.h "G.711"), checkable without a GPU: q3tts_g711_encode_host / _decode_host — the inline functions the
sink and encoder-stream kernels use — against the numpy restatement tests/g711_ref.py over every int16 value and every byte, the
properties the header states, the refusals, and the surface (header, exports, Python names, TTSEngine, the CLI's help).  What the
kernels compute is checked on the GPU: tests/test_gpu_g711_sink.py, test_gpu_g711_stream.py, test_gpu_cli_g711.py."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import g711_ref
import q3tts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAWS = ["mulaw", "alaw"]
ALL16 = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
ALL8 = np.arange(256, dtype=np.uint8)


@pytest.mark.parametrize("law", LAWS)
def test_encode_and_decode_equal_the_restatement_everywhere(law):
    enc = q3tts.g711_encode(law, ALL16)
    dec = q3tts.g711_decode(law, ALL8)
    assert enc.dtype == np.uint8 and dec.dtype == np.int16
    assert np.array_equal(enc, g711_ref.ENC[law](ALL16))
    assert np.array_equal(dec, g711_ref.DEC[law](ALL8))
    assert np.array_equal(q3tts.g711_encode(q3tts.PCM_MULAW if law == "mulaw" else q3tts.PCM_ALAW, ALL16), enc)
    assert q3tts.g711_encode(law, np.zeros(0, np.int16)).size == 0 and q3tts.g711_decode(law, np.zeros(0, np.uint8)).size == 0


@pytest.mark.parametrize("law", LAWS)
def test_properties_of_the_laws(law):
    enc = q3tts.g711_encode(law, ALL16)
    dec = q3tts.g711_decode(law, ALL8)
    rt = q3tts.g711_decode(law, enc).astype(np.int32)
    assert np.all(np.diff(rt) >= 0)                                            # decode(encode(s)) is monotone in s
    pos = np.arange(1, 32768, dtype=np.int32)
    assert np.array_equal(enc[32768 - pos], enc[32768 + pos] ^ 0x80)           # sign-magnitude: enc(-s) == enc(s) ^ 0x80
    back = q3tts.g711_encode(law, dec)
    differs = np.flatnonzero(back != ALL8)
    if law == "mulaw":
        assert differs.tolist() == [0x7F] and back[0x7F] == 0xFF               # negative zero re-encodes as silence
        assert enc[32768] == 0xFF and enc[0] == 0x00
        assert int(dec.max()) == 32124 and int(dec.min()) == -32124
    else:
        assert differs.size == 0
        assert enc[32768] == 0xD5 and enc[0] == 0x2A
        assert int(dec.max()) == 32256 and int(dec.min()) == -32256
    assert np.unique(enc).size == 256                                          # every code is reached (mu-law 0x7F by s = -1 .. -3)


def test_audioop_agreements():
    audioop = pytest.importorskip("audioop")
    raw16 = ALL16.astype("<i2").tobytes()
    for law, lin2, to_lin in (("mulaw", audioop.lin2ulaw, audioop.ulaw2lin), ("alaw", audioop.lin2alaw, audioop.alaw2lin)):
        theirs_dec = np.frombuffer(to_lin(ALL8.tobytes(), 2), "<i2")
        assert np.array_equal(q3tts.g711_decode(law, ALL8), theirs_dec)
        theirs_enc = np.frombuffer(lin2(raw16, 2), np.uint8)
        ours = q3tts.g711_encode(law, ALL16)
        assert np.array_equal(ours[32768:], theirs_enc[32768:])                # every s >= 0
        assert int((ours[:32768] != theirs_enc[:32768]).sum()) == (381 if law == "mulaw" else 127)


@pytest.mark.parametrize("law", LAWS)
def test_sine_sqnr(law):
    t = np.arange(8000, dtype=np.float64)
    x = (0.5 * np.sin(2.0 * np.pi * 1004.0 * t / 8000.0)).astype(np.float32)
    s = g711_ref.s16_rule(x)
    y = q3tts.g711_decode(law, q3tts.g711_encode(law, s)).astype(np.float64)
    sqnr = 10.0 * np.log10(np.sum(s.astype(np.float64) ** 2) / np.sum((y - s) ** 2))
    print("%s: SQNR %.2f dB" % (law, sqnr))
    assert sqnr >= 35.0


def test_other_formats_are_refused():
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for fn in (L.q3tts_g711_encode_host, L.q3tts_g711_decode_host):
        fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
        fn.restype = ctypes.c_int
    src16, dst8 = np.array([1, -1, 100], np.int16), np.full(3, 0x11, np.uint8)
    src8, dst16 = np.array([1, 2, 3], np.uint8), np.full(3, 0x1111, np.int16)
    for fmt in (0, 1, 4, 7, -1):
        assert L.q3tts_g711_encode_host(fmt, src16.ctypes.data, 3, dst8.ctypes.data) == -1
        assert L.q3tts_g711_decode_host(fmt, src8.ctypes.data, 3, dst16.ctypes.data) == -1
    assert (dst8 == 0x11).all() and (dst16 == 0x1111).all()                    # nothing was written
    assert L.q3tts_g711_encode_host(2, src16.ctypes.data, 3, dst8.ctypes.data) == 0
    assert dst8.tolist() == g711_ref.mu_enc(src16).tolist()
    assert L.q3tts_g711_encode_host(2, src16.ctypes.data, -1, dst8.ctypes.data) == -1
    for bad in ("float32", "int16", 0, 1, 7):
        with pytest.raises(ValueError):
            q3tts.g711_encode(bad, src16)
        with pytest.raises(ValueError):
            q3tts.g711_decode(bad, src8)
    with pytest.raises(ValueError, match="int16"):
        q3tts.g711_encode("mulaw", np.zeros(3, np.float32))
    with pytest.raises(ValueError, match="uint8"):
        q3tts.g711_decode("alaw", np.zeros(3, np.int16))


def test_header_exports_and_python_names():
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    assert re.search(r"#define\s+Q3TTS_PCM_MULAW\s+2\b", hdr) and re.search(r"#define\s+Q3TTS_PCM_ALAW\s+3\b", hdr)
    assert re.search(r"#define\s+Q3TTS_PCM_F32\s+0\b", hdr) and re.search(r"#define\s+Q3TTS_PCM_S16\s+1\b", hdr)
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for name in ("q3tts_g711_encode_host", "q3tts_g711_decode_host", "q3tts_read_wav_g711_host"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in q3tts.EXPORTS and hasattr(L, name), name
    assert "int q3tts_g711_encode_host(int format, const int16_t* in, int64_t n, uint8_t* out);" in hdr
    assert "int q3tts_g711_decode_host(int format, const uint8_t* in, int64_t n, int16_t* out);" in hdr
    for word in ("32635", "132", "0x55", "0xD5", "0xFF", "0x7F"):                # the arithmetic stands in the header
        assert word in hdr, word
    assert (q3tts.PCM_F32, q3tts.PCM_S16, q3tts.PCM_MULAW, q3tts.PCM_ALAW) == (0, 1, 2, 3)


def test_pcm_format_names_and_pinned_refusals():
    assert q3tts._pcm_format("mulaw") == 2 and q3tts._pcm_format("ulaw") == 2 and q3tts._pcm_format("alaw") == 3
    assert q3tts._pcm_format("float32") == 0 and q3tts._pcm_format(np.int16) == 1 and q3tts._pcm_format("int16") == 1
    with pytest.raises(ValueError, match="dtype must be float32 or int16"):
        q3tts._pcm_format("int32")
    with pytest.raises(ValueError, match="dtype must be float32 or int16"):
        q3tts._pcm_format(np.uint8)                                            # a byte array names no law
    src = lambda name: open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", name)).read()
    assert 'format must be Q3TTS_PCM_F32 (0) or Q3TTS_PCM_S16 (1), got " + std::to_string(format)' in src("q3_encoder.cpp")
    for name in ("q3_pcm_sink.cpp", "q3_codec.cpp", "q3_capi.cpp"):
        assert " is neither Q3TTS_PCM_F32 nor Q3TTS_PCM_S16" in src(name), name


def test_tts_engine_declares_old_and_new_members():
    h = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "tts_engine.h")).read()
    flat = re.sub(r"\s+", " ", h)
    for old in ("bool set_output_format(int sample_rate, bool pcm16 = false);",
                "bool convert_output(const std::vector<float>& pcm24, std::vector<float>* f32, std::vector<int16_t>* s16);",
                "bool pcm16 = false);",
                "std::vector<int64_t> audio_stream_push(int id, const int16_t* pcm, size_t n, bool finish = false, bool* ok = nullptr);",
                "bool output_pcm16() const"):
        assert old in flat, old
    assert re.search(r"int audio_stream_begin\(int64_t max_samples, int sample_rate[^)]*, bool pcm16 = false\);", flat)
    for new in ("bool set_output_encoding(int sample_rate, int format);", "int output_encoding() const",
                "std::vector<uint8_t>* g711);",
                "int audio_stream_begin_encoded(int64_t max_samples, int sample_rate, int format);",
                "std::vector<int64_t> audio_stream_push(int id, const uint8_t* pcm, size_t n, bool finish = false, bool* ok = nullptr);"):
        assert new in flat, new


def test_cli_source_knows_the_flag_and_the_wav_layout():
    m = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "main.cpp")).read()
    assert "--out-format" in m and "mulaw" in m and "alaw" in m and "pcm16" in m
    assert '"fact"' in m and "read_wav_g711" in m
    a = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "q3_audio.h")).read()
    assert "read_wav_g711(const std::string& path, int* sample_rate, int* format)" in a


def _g711_wav(path, tag, channels, rate, data, bits=8):
    pad = len(data) & 1
    body = b"WAVE" + b"fmt " + struct.pack("<IHHIIHHH", 18, tag, channels, rate, rate * channels, channels, bits, 0)
    body += b"fact" + struct.pack("<II", 4, len(data) // channels) + b"data" + struct.pack("<I", len(data)) + data + b"\0" * pad
    open(path, "wb").write(b"RIFF" + struct.pack("<I", len(body)) + body)


def test_read_wav_g711_host(tmp_path):
    L = ctypes.CDLL(q3tts.LIB_PATH)
    fn = L.q3tts_read_wav_g711_host
    fn.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int)]
    fn.restype = ctypes.c_int

    def read(path):
        n, sr, fmt = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int(0)
        rc = fn(os.fsencode(path), None, 0, ctypes.byref(n), ctypes.byref(sr), ctypes.byref(fmt))
        if rc != 0:
            return rc
        out = np.zeros(n.value, np.uint8)
        assert fn(os.fsencode(path), out.ctypes.data, out.size, ctypes.byref(n), ctypes.byref(sr), ctypes.byref(fmt)) == 0
        return out, sr.value, fmt.value

    data = np.random.default_rng(0).integers(0, 256, 1001).astype(np.uint8)
    for tag, fmt in ((7, q3tts.PCM_MULAW), (6, q3tts.PCM_ALAW)):
        p = str(tmp_path / ("g%d.wav" % tag))
        _g711_wav(p, tag, 1, 8000, data.tobytes())                             # odd length: the pad byte is not a sample
        got, sr, f = read(p)
        assert np.array_equal(got, data) and sr == 8000 and f == fmt
        assert q3tts.read_wav(p) is None                                       # the reference's reader refuses it, as before
    stereo = str(tmp_path / "stereo.wav")
    _g711_wav(stereo, 7, 2, 8000, data[:1000].tobytes())
    assert read(stereo) == -2
    wide = str(tmp_path / "wide.wav")
    _g711_wav(wide, 7, 1, 8000, data.tobytes(), bits=16)
    assert read(wide) == -1
    pcm = str(tmp_path / "pcm.wav")
    _g711_wav(pcm, 1, 1, 8000, data.tobytes())
    assert read(pcm) == -1 and read(str(tmp_path / "missing.wav")) == -1
