"""The packed-rows layer (mdctgan_amd/packed.py) without a GPU: the one alignment rule, the window table, the one-copy upload,
and the two host restatements that lean on them -- resample_length against the library's mg_resample_length, and
plan_utterances / plan_front_end agreeing on where the final buffer's utterances lie.
"""
import numpy as np
import pytest
import torch

LENGTHS = [1, 63, 64, 65]
RATE_PAIRS = [(48000, 8000), (8000, 48000), (44100, 48000)]
RESAMPLE_LENGTHS = [1, 7, 4097]


@pytest.mark.parametrize("align, starts, total", [(1, [0, 1, 64, 128], 193), (64, [0, 64, 128, 192], 320)])
def test_aligned_layout(align, starts, total):
    from mdctgan_amd.packed import PackedLayout, aligned_layout
    lay = aligned_layout(LENGTHS, align)
    assert isinstance(lay, PackedLayout) and lay.lengths == LENGTHS
    assert lay.starts == starts and lay.total == total
    assert all(s % align == 0 for s in lay.starts) and lay.total % align == 0
    # the gap rule: every start (and the total) is the first multiple of `align` at or after the end of the one before
    ends = [s + n for s, n in zip(lay.starts, lay.lengths)]
    assert lay.starts[0] == 0
    assert all(0 <= nxt - end < align for end, nxt in zip(ends, lay.starts[1:] + [lay.total]))


def test_aligned_layout_default_is_64():
    from mdctgan_amd.packed import aligned_layout
    assert aligned_layout(LENGTHS) == aligned_layout(LENGTHS, 64)


def test_window_table():
    from mdctgan_amd.packed import window_table
    starts, lengths = [0, 64, 128, 192], LENGTHS
    t = window_table(starts, lengths)
    assert t.dtype == np.int64 and t.shape == (4, 3)
    assert t.tolist() == [[0, 0, 1], [64, 64, 127], [128, 128, 192], [192, 192, 257]]
    order = [2, 0, 3, 1]
    assert window_table(starts, lengths, order).tolist() == [t[u].tolist() for u in order]
    assert window_table(starts, lengths, range(4)).tolist() == t.tolist()


def test_upload_tables_is_one_storage_in_the_parts_own_shapes():
    from mdctgan_amd.packed import upload_tables
    parts = [np.arange(12, dtype=np.int64).reshape(4, 3) * 7, np.arange(5, dtype=np.int64) - 2,
             np.arange(8, dtype=np.int64).reshape(2, 4) + 100]
    views = upload_tables(parts, "cpu")
    assert len(views) == 3
    for v, p in zip(views, parts):
        assert v.dtype == torch.int64 and tuple(v.shape) == p.shape and v.is_contiguous()
        assert np.array_equal(v.numpy(), p)
    base = views[0].untyped_storage().data_ptr()
    assert all(v.untyped_storage().data_ptr() == base for v in views)
    assert views[0].untyped_storage().nbytes() == 8 * sum(p.size for p in parts)
    assert [v.storage_offset() for v in views] == [0, 12, 17]
    # a list travels as an int64 array too (plan.frame_start)
    only, = upload_tables([[3, 1, 2]], "cpu")
    assert only.dtype == torch.int64 and only.tolist() == [3, 1, 2]


@pytest.mark.parametrize("orig, new", RATE_PAIRS)
def test_resample_length_is_the_librarys(orig, new):
    import math

    from mdctgan_amd import _lib
    from mdctgan_amd.resample import resample_length
    lib, g = _lib.load(), math.gcd(orig, new)
    for L in RESAMPLE_LENGTHS:
        assert resample_length(L, orig, new) == lib.mg_resample_length(L, orig // g, new // g) == -(-new * L // orig)
    for bad in ((0, orig, new), (5, 0, new), (5, orig, -1)):
        assert lib.mg_resample_length(*bad) == -1
        with pytest.raises(ValueError):
            resample_length(*bad)


@pytest.mark.parametrize("orig, new", RATE_PAIRS)
@pytest.mark.parametrize("align", [1, 64])
def test_plans_agree_on_the_final_buffer(orig, new, align):
    from mdctgan_amd.generate_audio import plan_utterances
    from mdctgan_amd.packed import aligned_layout
    from mdctgan_amd.resample import plan_front_end, resample_length
    plan = plan_front_end(RESAMPLE_LENGTHS, [orig] * 3, new, new, True, 4096, 0, 8, align=align)
    final = [resample_length(L, orig, new) for L in RESAMPLE_LENGTHS]
    utt = plan_utterances(final, 4096, 4096, 0, 8, align)
    assert plan.final_lengths == final
    assert plan.starts[-1] == utt.in_start and plan.totals[-1] == utt.in_total
    assert utt.in_layout == aligned_layout(final, align) == plan.utterances.in_layout
    assert (plan.starts[0], plan.totals[0]) == (aligned_layout(RESAMPLE_LENGTHS, align).starts,
                                                aligned_layout(RESAMPLE_LENGTHS, align).total)
