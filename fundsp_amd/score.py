"""Scores for a pool of voices (Bank.set_score): host-side helpers, numpy only, no device."""
import heapq

import numpy as np


def assign_voices(start, end, polyphony):
    """Allot the notes (start[k], end[k]) to `polyphony` voices so that no voice plays two notes at once.

    Notes are taken in order of start, ties broken by index; each goes to the lowest-numbered voice whose last note has
    end <= start (legato reuses a voice).  Returns the voice per note (int32, in the order given) -- a result that always
    satisfies the overlap rule of Bank.set_score.  Raises ValueError naming the first note that does not fit."""
    start = np.atleast_1d(np.asarray(start, dtype=np.float64))
    end = np.atleast_1d(np.asarray(end, dtype=np.float64))
    if start.shape != end.shape or start.ndim != 1:
        raise ValueError("start and end must be one-dimensional and of one length")
    polyphony = int(polyphony)
    if polyphony < 0:
        raise ValueError("polyphony must not be negative")
    if start.size and not np.all(end >= start):
        raise ValueError(f"note {int(np.flatnonzero(~(end >= start))[0])} ends before it starts")
    voice = np.empty(start.size, dtype=np.int32)
    free = list(range(polyphony))  # min-heap of the voices that are free now
    busy = []                      # min-heap of (end, voice) of the sounding ones
    for k in np.argsort(start, kind="stable"):
        while busy and busy[0][0] <= start[k]:
            heapq.heappush(free, heapq.heappop(busy)[1])
        if not free:
            raise ValueError(f"note {int(k)} (start {start[k]!r}) does not fit: all {polyphony} voices are sounding")
        v = heapq.heappop(free)
        voice[k] = v
        heapq.heappush(busy, (float(end[k]), v))
    return voice
