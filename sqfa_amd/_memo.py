"""Memoisation of values derived from tensors, per tensor OBJECT and version."""
import weakref


class TensorMemo:
    """value = f(tensors...) remembered for exactly these tensor objects at their current ``_version``.

    Keyed by ``id`` and checked through a weak reference, never by address: the caching allocator hands a freed address
    to the next tensor, and Python hands a dead object's id to the next object, so a hit needs the SAME live object(s).
    An in-place edit (a new ``_version``) misses.  The entry is dropped as soon as any key tensor dies; `max_entries`,
    when given, bounds the live entries (the oldest goes first).  Keys that cannot be weakly referenced are not stored.
    Values must not be None (None is the miss)."""

    def __init__(self, max_entries=None):
        self.max_entries = max_entries
        self._entries = {}   # ids -> (weak references, versions, value)

    def __len__(self):
        return len(self._entries)

    def get(self, *tensors):
        hit = self._entries.get(tuple(map(id, tensors)))
        if (hit is not None and all(ref() is t for ref, t in zip(hit[0], tensors))
                and hit[1] == tuple(getattr(t, "_version", None) for t in tensors)):
            return hit[2]
        return None

    def put(self, value, *tensors):
        key = tuple(map(id, tensors))
        entries = self._entries
        try:
            refs = tuple(weakref.ref(t, lambda _r: entries.pop(key, None)) for t in tensors)
        except TypeError:
            return value
        entries.pop(key, None)   # a re-put moves to the young end
        entries[key] = (refs, tuple(getattr(t, "_version", None) for t in tensors), value)
        while self.max_entries is not None and len(entries) > self.max_entries:
            entries.pop(next(iter(entries)))
        return value
