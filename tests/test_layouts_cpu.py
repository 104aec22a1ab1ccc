"""The per-module cache of derived weight layouts (sgm.modules.hipnn.layout) on small CPU modules: a hit is the same object, a
version bump or a new pointer of each declared source rebuilds the layout and nothing else does, a frozen owner serves what it
built and refuses the rest with UdtError, layouts die with their module, and drop_layouts leaves frozen owners alone."""
import gc
import weakref

import pytest
import torch

import udifftext_amd  # noqa: F401
from sgm.modules import hipnn as H
from sgm.modules.attention import GEGLU, CrossAttention
from sgm.modules.encoders.modules import _EncoderLayer
from udifftext_amd.lib import UdtError


def _bump(t):
    with torch.no_grad():
        t.mul_(1.0)                     # same values, _version + 1


def _linear():
    m = H.Linear(64, 32)
    return m, m.packed, [m.weight, m.bias], []


def _geglu_ln():
    m, ln = GEGLU(64, 32), H.LayerNorm(64)
    return m, lambda: m.packed_ln(ln), [m.proj.weight, m.proj.bias, ln.weight, ln.bias], []


def _cross_attention():
    m = CrossAttention(64, context_dim=32, heads=2, dim_head=32)
    return m, m.packed, [m.to_k.weight, m.to_v.weight], [m.to_q.weight, m.to_out[0].weight, m.to_out[0].bias]


def _encoder_layer():
    m = _EncoderLayer(64, 2, 128)
    a = m.self_attn
    return m, m.packed, [a.in_proj_weight, a.in_proj_bias], [a.out_proj.weight, m.linear1.weight, m.norm1.weight]


CASES = [_linear, _geglu_ln, _cross_attention, _encoder_layer]


@pytest.mark.parametrize("make", CASES, ids=lambda f: f.__name__.strip("_"))
def test_layout_follows_exactly_its_sources(make):
    mod, get, sources, others = make()
    pk = get()
    assert get() is pk                                          # a hit is the cached object
    for p in others:                                            # inputs of other layouts do not rebuild this one
        _bump(p)
        assert get() is pk
    for p in sources:                                           # each declared source does
        _bump(p)
        new = get()
        assert new is not pk and get() is new
        pk = new
    with torch.no_grad():                                       # so does a new pointer (load, .to(), reassignment)
        sources[0].data = sources[0].data.clone()
    assert get() is not pk


def test_encoder_layer_bias_update_reaches_its_pack():
    m = _EncoderLayer(64, 2, 128)
    _, b = m.packed()
    with torch.no_grad():
        m.self_attn.in_proj_bias.add_(1.0)
    assert torch.equal(m.packed()[1], b + 1.0)


def test_conv_segments_are_part_of_the_key():
    conv = H.Conv2d(16, 32, 3, padding=1)
    w0, _ = conv.packed()
    conv.segments = (8, 8)
    w1, _ = conv.packed()
    assert w1.shape[1] == 2 * w0.shape[1]                      # (each source padded to 64 channels on its own)
    assert conv.packed()[0] is w1


def test_frozen_owner_serves_built_layouts_and_refuses_the_rest():
    m, ln = GEGLU(64, 32), H.LayerNorm(64)
    pk = m.packed()
    H.freeze_layouts(m)
    for p in m.proj.parameters():                               # what prepare(free_masters=True) does to the masters
        p.data = torch.empty(0)
    assert m.packed() is pk
    with pytest.raises(UdtError, match=r"GEGLU: layout 'ln'"):
        m.packed_ln(ln)
    lin = H.Linear(64, 32)
    H.freeze_layouts(lin)
    for get, tag in ((lin.packed, "plain"), (lin.packed_fp8, "fp8")):
        with pytest.raises(UdtError, match=f"Linear: layout '{tag}'"):
            get()


def test_layouts_die_with_their_module():
    m = H.Linear(64, 32)
    ref = weakref.ref(m.packed()[0])
    mod = weakref.ref(m)
    del m
    gc.collect()
    assert mod() is None and ref() is None


def test_drop_layouts_keeps_frozen_owners():
    a, b = H.Linear(64, 32), H.Linear(32, 16)
    root = torch.nn.Sequential(a, b)
    pa, pb = a.packed(), b.packed()
    H.freeze_layouts(a)
    H.drop_layouts(root)
    assert H.has_layout(a, "plain") and not H.has_layout(b, "plain")
    assert a.packed() is pa and b.packed() is not pb
