"""Argument checks that several modules share word for word.  A check lives here only if every caller accepts the same values,
gets the same value back and raises the same message; checks that differ in any of the three stay in their modules."""
import math

import numpy as np

MAX_ITEMS = 2 ** 31 - 1   # rows, vertices, triangles: what the C ABI's int64 counts take


def count(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= MAX_ITEMS:
        raise ValueError("%s must be an integer in [0, 2^31 - 1], got %r" % (what, v))
    return int(v)


def whole(v, what, least):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < least:
        raise ValueError("%s must be an integer >= %d, got %r" % (what, least, v))
    return int(v)


def positive(v, what):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError("%s must be a finite number > 0, got %r" % (what, v))
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError("%s must be a finite number > 0, got %r" % (what, v))
    return v


def colour_words(rgba, n, what="rgba"):
    w = np.asarray(rgba)
    if w.dtype != np.uint32 or w.ndim != 1 or w.shape[0] != n:
        raise ValueError("%s must be [N] uint32 colour words (r | g << 8 | b << 16), one per point: got %s %s for %d points"
                         % (what, w.dtype, w.shape, n))
    return np.ascontiguousarray(w)
