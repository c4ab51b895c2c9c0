"""Restatement, in plain Python / numpy, of what the reference's Python does to a 1D read once load_from_raw2 has written its
basecalled event table: NanoporeRead.make_event_map (src/signalalign/nanoporeRead.py:313-333) and the fourteen lines of
NanoporeRead.Write (:438-540).  The table comes from sa_raw_event_align_batch on the GPU (tests/test_gpu_raw_npread.py) or
from tests/event_detect_ref.py + the C oracle on the CPU (tests/test_host_raw_npread.py)."""
import numpy as np


def make_event_map(move, p_model_state, k):
    """One entry per base of the read: the row (event) that base starts in.  Row 0 opens the map whatever its move; the
    probability a move-0 row is compared with is the previous ROW's, and 0 for row 1 (previous_prob starts at 0 and is
    first assigned at the end of row 1's turn)."""
    event_map = [0]
    previous_prob = 0
    for i in range(1, len(move)):
        mv = int(move[i])
        this_prob = float(p_model_state[i])
        if mv == 1:
            event_map.append(i)
        if mv > 1:
            for _ in range(mv - 1):
                event_map.append(i - 1)
            event_map.append(i)
        if mv == 0:
            if this_prob > previous_prob:
                event_map[-1] = i
        previous_prob = this_prob
    return event_map + [event_map[-1]] * (k - 1)


def mapped_rows(events):
    """the rows the reference writes: sa_raw_event_align_batch's events (RAW_EVENT_DTYPE, time order) with a k-mer"""
    return events[events["kmer_idx"] >= 0]


def events4_of(rows):
    """the .npRead's four columns: mean, stdv, length, start - start of row 0"""
    return np.stack([rows["mean"], rows["stdv"], rows["length"], rows["start"] - rows["start"][0]], axis=1)


def npread_text(sequence, rows, k):
    """NanoporeRead.Write for a 1D read whose template events are `rows`: no 2D read, the strand parameters at their defaults
    (1 1 1 1 1 0 twice, has-2D 0), an empty complement; print(x, end=' ') leaves a blank after every list entry, and a
    float64 prints as its repr."""
    def ints(v):
        return "".join("%d " % x for x in v)

    def floats(v):
        return "".join(repr(float(x)) + " " for x in v)
    ev_map = make_event_map(rows["move"], rows["p_model_state"], k)
    lines = [
        "0 %d 0 %d 0 1 1 1 1 1 0 1 1 1 1 1 0 0" % (len(rows), len(sequence)),
        "",                                  # 2  alignment table sequence (2D read)
        sequence,                            # 3  template read
        ints(ev_map),                        # 4  template strand map
        "",                                  # 5  complement read
        "",                                  # 6  complement strand map
        "",                                  # 7  template 2D event map
        floats(events4_of(rows).reshape(-1)),  # 8  template events
        "",                                  # 9  complement 2D event map
        "",                                  # 10 complement events
        "".join(sequence[x:x + k] + " " for x in rows["kmer_idx"].tolist()),   # 11 model states
        floats(rows["p_model_state"]),       # 12 their probabilities
        "",                                  # 13, 14: the complement's
        "",
    ]
    return "\n".join(lines) + "\n"
