"""The one rule for a buffer that rides on the tensor it mirrors (functional._attach / _sidecar): the record is
(buffer, data_ptr, _version, key), and it is trusted only while the tensor is the one it was made from -- same storage address, same
version counter, the key the consumer expects, channels_last contiguous.  CPU tensors; all three attribute names."""
import pytest
import torch

from mdctgan_amd import functional as Fh

CL = torch.channels_last
# attribute, the key its users give it, the counter its producers are counted in
KINDS = [("_mg_h16", lambda t: t.numel(), Fh.H16_STATS),
         ("_mg_h16_rows", lambda t: 2, Fh.H16_STATS),
         ("_mg_wino_v", lambda t: (4, 6, 10, 8, True, 0, 16), Fh.WINO_NEXT_STATS)]


def _tensor():
    return torch.randn(4, 8, 6, 10).contiguous(memory_format=CL)


@pytest.mark.parametrize("attr,key_of,stats", KINDS, ids=[k[0] for k in KINDS])
def test_sidecar_rule(attr, key_of, stats):
    t, buf = _tensor(), torch.zeros(7, dtype=torch.float16)
    key, made = key_of(t), stats["made"]
    assert Fh._attach(t, attr, buf, key) is t
    assert stats["made"] == made + 1
    rec = getattr(t, attr)
    assert isinstance(rec, tuple) and len(rec) == 4 and rec[0] is buf and rec[1:] == (t.data_ptr(), t._version, key)
    assert Fh._sidecar(t, attr, key) is buf
    assert Fh._sidecar(t, attr, key) is buf                     # looking does not use it up
    # another key
    other = key + 1 if isinstance(key, int) else key[:-1] + (36,)
    assert Fh._sidecar(t, attr, other) is None
    # another tensor: a clone carries no record, and the record on another storage is not believed
    c = t.clone()
    assert Fh._sidecar(c, attr, key) is None
    setattr(c, attr, rec)
    assert Fh._sidecar(c, attr, key) is None
    # not channels_last contiguous (same storage, same version: only the layout differs)
    n = torch.randn(4, 8, 6, 10)
    Fh._attach(n, attr, buf, key_of(n))
    assert stats["made"] == made + 2
    assert not n.is_contiguous(memory_format=CL) and Fh._sidecar(n, attr, key_of(n)) is None
    # an in-place write
    t.add_(1.0)
    assert Fh._sidecar(t, attr, key) is None
    # nothing to hang: no record, no count
    e = _tensor()
    assert Fh._attach(e, attr, None, key) is e and not hasattr(e, attr) and stats["made"] == made + 2
    assert Fh._sidecar(e, attr, key) is None


def test_default_key_is_the_element_count():
    t, buf = _tensor(), torch.zeros(3, dtype=torch.float16)
    made = Fh.H16_STATS["made"]
    assert Fh._attach(t, "_mg_h16", buf) is t and Fh.H16_STATS["made"] == made + 1
    assert t._mg_h16[0] is buf and t._mg_h16[1:] == (t.data_ptr(), t._version, t.numel()) and Fh._sidecar(t, "_mg_h16") is buf
    half = t[:2]
    half._mg_h16 = t._mg_h16                                    # same address, same version: the element count tells them apart
    assert Fh._sidecar(half, "_mg_h16") is None and Fh._sidecar(t.clone(), "_mg_h16") is None
