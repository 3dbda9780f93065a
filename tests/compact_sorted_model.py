"""What evql_lsm_chain_compact_sorted must write, as a model in numpy: the columns
compact_model.expected_columns gives for the plain compaction, every one of them reordered
by np.argsort(key words, kind="stable") -- ascending as unsigned 64-bit words, equal keys in
the plain compaction's order -- and fed to the host writer E.Writer as
compact_model.expected_image does."""
import numpy as np

import eventql_amd as E
import compact_model as M


def key_words(specs, cols, key):
    c = cols[[s["name"] for s in specs].index(key)]
    return np.asarray(c["values"], np.uint64)


def _permuted(values, perm):
    if isinstance(values, list):
        return [values[i] for i in perm]
    return np.asarray(values)[perm]


def sorted_columns(out_specs, plain_cols, key):
    """the columns of the plain compaction (compact_model.expected_columns) in key order:
    (columns, the stable permutation); plain_cols is left as it is"""
    perm = np.argsort(key_words(out_specs, plain_cols, key), kind="stable")
    out = []
    for c in plain_cols:
        if c["rl"] is not None or c["dl"] is not None:
            raise ValueError("rows of a repeated / nested column do not move alone")
        out.append(dict(values=_permuted(c["values"], perm),
                        present=None if c["present"] is None else c["present"][perm],
                        rl=None, dl=None))
    return out, perm


def image_of(out_specs, cols, rows):
    """the file bytes E.Writer makes of flat columns"""
    w = E.Writer(out_specs)
    for spec, c in zip(out_specs, cols):
        w.put(spec["name"], c["values"], rlvl=None, dlvl=None, present=c["present"])
    w.commit(rows)
    img = w.image()
    w.close()
    return img


def expected_columns(files_oldest_first, out_specs, key, row_order, filters=None):
    """(per output column dict(values, present, rl, dl), output rows, the stable permutation)"""
    plain, rows = M.expected_columns(files_oldest_first, out_specs, row_order, filters)
    cols, perm = sorted_columns(out_specs, plain, key)
    return cols, rows, perm


def expected_image(files_oldest_first, out_specs, key, row_order, filters=None):
    cols, rows, _ = expected_columns(files_oldest_first, out_specs, key, row_order, filters)
    return image_of(out_specs, cols, rows)


def expected_passes(keys):
    """(presorted, passes, key_min, key_max) as evql_compact_sort_stats_t reports them"""
    keys = np.asarray(keys, np.uint64)
    if len(keys) == 0:
        return 1, 0, 0, 0
    lo, hi = int(keys.min()), int(keys.max())
    if len(keys) <= 1 or not (keys[1:] < keys[:-1]).any():
        return 1, 0, lo, hi
    return 0, ((hi - lo).bit_length() + 7) // 8, lo, hi
