"""The surface of the b = 1 predictor's QKV table, checkable without a GPU: the built library holds the sampler variant that copies a
table row (one instantiation beside the plain samplers, no scratch segment) and the widening kernel of the table builder; the knob is
documented.  (What the table path computes is checked on the GPU: tests/test_gpu_cp_qkv_table.py.)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_library_holds_the_table_sampler():
    import q3tts
    from kernel_resources import kernel_table
    rows = [(name, scratch) for name, vgpr, agpr, sgpr, scratch, lds in kernel_table(q3tts.LIB_PATH)]
    samplers = [(n, s) for n, s in rows if "k_sample<" in n]
    tab = [(n, s) for n, s in samplers if n.split("(")[0].replace(" ", "").endswith(",true>") and "<false,8,false,true>" in n.replace(" ", "")]
    assert len(tab) == 1, samplers
    assert len(samplers) == 10, samplers          # 9 plain (slabs | penalty | neither, x 3 widths) + the table copy
    assert all(s == 0 for _, s in samplers), samplers
    conv = [(n, s) for n, s in rows if "k_bf16_to_f32" in n]
    assert len(conv) == 1 and conv[0][1] == 0, conv


def test_knob_is_documented():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Q3TTS_CP_QKV_TABLE" in doc
