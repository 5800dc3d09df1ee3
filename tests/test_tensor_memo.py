"""CPU tests of sqfa_amd._memo.TensorMemo: values remembered per tensor OBJECT and version."""
import gc

import torch

from sqfa_amd._memo import TensorMemo


def test_same_objects_hit_and_edits_or_other_tensors_miss():
    memo = TensorMemo()
    a, b = torch.zeros(3), torch.ones(3)
    assert memo.get(a) is None and memo.get(a, b) is None
    assert memo.put("A", a) == "A" and memo.put("AB", a, b) == "AB"
    assert memo.get(a) == "A" and memo.get(a, b) == "AB"
    assert memo.get(b) is None and memo.get(b, a) is None and memo.get(a.clone()) is None
    assert memo.get(a.view(3)) is None                     # another object on the same storage
    b.add_(1.0)                                            # in-place edit of ONE key: a new version
    assert memo.get(a, b) is None and memo.get(a) == "A"
    memo.put(False, a)                                     # False is a value (the symmetry verdict), None is the miss
    assert memo.get(a) is False


def test_entry_dies_with_any_key_tensor():
    memo = TensorMemo()
    a, b, c = torch.zeros(2), torch.zeros(2), torch.zeros(2)
    memo.put(1, a, b)
    memo.put(2, c)
    assert len(memo) == 2
    del b
    gc.collect()
    assert len(memo) == 1 and memo.get(c) == 2
    del c
    gc.collect()
    assert len(memo) == 0


def test_stale_entry_is_never_returned_for_a_new_object_with_the_same_id():
    """Python hands a dead object's id to the next object: with the death callback gone (as after a lost race), the
    entry under that id still fails the identity check of its weak reference."""
    memo = TensorMemo()
    a = torch.zeros(2)
    memo.put("old", a)
    key = (id(a),)
    entry = memo._entries[key]
    del a
    gc.collect()
    assert key not in memo._entries
    fresh = torch.zeros(2)
    memo._entries[(id(fresh),)] = entry                    # the dead tensor's entry under the live tensor's id
    assert memo.get(fresh) is None
    ids = set()
    for _ in range(200):                                   # real id reuse: short-lived tensors share a few ids
        t = torch.zeros(2)
        assert memo.get(t) is None
        memo.put("x", t)
        ids.add(id(t))
        del t
    assert len(ids) < 200 and len(memo) == 1             # ids were reused; only the planted entry is left


def test_bound_keeps_the_youngest_entries():
    memo = TensorMemo(max_entries=4)
    tensors = [torch.zeros(1) for _ in range(7)]
    for i, t in enumerate(tensors):
        memo.put(i, t)
    assert len(memo) == 4
    assert [memo.get(t) for t in tensors] == [None, None, None, 3, 4, 5, 6]


def test_keys_without_weak_references_are_not_stored():
    memo = TensorMemo()
    assert memo.put("v", 3) == "v" and memo.put("w", torch.zeros(1), (1, 2)) == "w"
    assert len(memo) == 0 and memo.get(3) is None
