"""What evql_lsm_chain_compact must write, as a model in numpy: the rows (records) the
partition cursor's filters keep, table after table, under the column rules of
include/evql_gpu.h, fed to the product's host writer E.Writer (pinned byte-identical to the
reference's CSTableWriter in test_format_cpu.py).

A partition is a list of files OLDEST first, (name, image, has_skiplist, has_updates, cols)
as tests/lsm_tables.py and tests/lsm_nested_tables.py build them.  `cols` describes the
file's columns either by the keys those modules use or, for hand-built files, by
cols["columns"] = {name: dict(values, present=None, rl=None, dl=None, rec_of_slot=None,
logical_type, rlevel_max, dlevel_max)}."""
import numpy as np

import eventql_amd as E
from eventql_amd import capi as K
import lsm_tables

SCAN_ORDER, FILE_ORDER = K.COMPACT_SCAN_ORDER, K.COMPACT_FILE_ORDER


def _col(values, logical_type, present=None, rl=None, dl=None, rec_of_slot=None, rlevel_max=0,
         dlevel_max=0):
    return dict(values=values, present=present, rl=rl, dl=dl, rec_of_slot=rec_of_slot,
                logical_type=logical_type, rlevel_max=rlevel_max, dlevel_max=dlevel_max)


def columns_of(cols, file_index, has_skiplist):
    """the columns of one file: name -> _col(...)"""
    if "columns" in cols:
        return cols["columns"]
    n = len(cols["ids"])
    i = np.arange(n, dtype=np.uint64)
    U, B, S, F = K.COL_UNSIGNED_INT, K.COL_BOOLEAN, K.COL_STRING, K.COL_FLOAT
    out = {"__lsm_is_update": _col(cols["upd"], B),
           "__lsm_id": _col(cols["ids"], S),
           "__lsm_version": _col(i + np.uint64(1), U),
           "__lsm_sequence": _col(i + np.uint64(file_index * 1_000_000 + 1), U)}
    if has_skiplist:
        out["__lsm_skip"] = _col(cols["skip"], B)
    if "rid" in cols:  # lsm_tables
        out.update(rid=_col(cols["rid"], U), k=_col(cols["k"], U), a=_col(cols["a"], U),
                   n=_col(cols["n"], U, present=cols["n_present"], dlevel_max=1),
                   v=_col(cols["v"], F), s=_col(cols["s"], S))
    else:              # lsm_nested_tables
        total = len(cols["pos"])
        rl = np.ones(total, np.uint64)
        rl[cols["starts"]] = 0
        dl = np.where(cols["defined"], 2, 0).astype(np.uint64)
        out.update(id=_col(cols["id"], U), k=_col(cols["k"], U), s=_col(cols["s"], S))
        for name, key in (("items.position", "pos"), ("items.price", "price")):
            out[name] = _col(cols[key], U, rl=rl, dl=dl, rec_of_slot=cols["rec_of_slot"],
                             rlevel_max=1, dlevel_max=2)
    return out


def _take(values, mask):
    if isinstance(values, list):
        return [v for v, m in zip(values, mask) if m]
    return np.asarray(values)[mask]


def expected_columns(files_oldest_first, out_specs, row_order, filters=None):
    """(per output column dict(values, present, rl, dl), output rows); filters: bool arrays
    in SCAN order or None per file (default: lsm_tables.model_filters)"""
    if filters is None:
        filters = lsm_tables.model_filters(files_oldest_first)
    n = len(files_oldest_first)
    tabs = [(n - 1 - k, f, filters[k]) for k, f in enumerate(reversed(files_oldest_first))]
    if row_order == FILE_ORDER:
        tabs.reverse()
    elif row_order != SCAN_ORDER:
        raise ValueError("bad row order")
    out = [dict(values=[], present=[], rl=[], dl=[]) for _ in out_specs]
    rows = 0
    for fi, f, flt in tabs:
        cols = columns_of(f[4], fi, f[2])
        nrec = len(f[4]["ids"])
        keep = np.ones(nrec, bool) if flt is None else np.asarray(flt, bool)
        nk = int(keep.sum())
        rows += nk
        for spec, o in zip(out_specs, out):
            name = spec["name"]
            is_str = spec["logical_type"] == K.COL_STRING
            rmax, dmax = spec.get("rlevel_max", 0), spec.get("dlevel_max", 0)
            nested = rmax > 0 or dmax > 1
            if name == "__lsm_skip":
                raise ValueError("a compacted table has no skiplist")
            c = cols.get(name)
            if name == "__lsm_is_update":
                vals, pres, rl, dl = np.zeros(nk, np.uint64), np.ones(nk, np.uint8), None, None
            elif c is None:
                if dmax == 0:
                    raise ValueError("can't merge CSTables after a new required column was added")
                vals = [b""] * nk if is_str else np.zeros(nk, np.uint64)
                pres = np.zeros(nk, np.uint8)
                rl = dl = np.zeros(nk, np.uint64)  # one (0, 0) slot per kept record
            else:
                if (c["logical_type"], c["rlevel_max"], c["dlevel_max"]) != \
                        (spec["logical_type"], rmax, dmax):
                    raise ValueError("column type or levels differ")
                if nested:
                    ros = np.arange(nrec) if c["rec_of_slot"] is None else c["rec_of_slot"]
                    sm = keep[ros]
                    vals = _take(c["values"], sm)
                    rl = np.zeros(int(sm.sum()), np.uint64) if c["rl"] is None else c["rl"][sm]
                    dl, pres = c["dl"][sm], None
                else:
                    vals = _take(c["values"], keep)
                    pres = np.ones(nk, np.uint8) if c["present"] is None else \
                        np.asarray(c["present"], np.uint8)[keep]
                    rl = dl = None
            o["values"].append(vals)
            o["present"].append(pres)
            o["rl"].append(rl)
            o["dl"].append(dl)
    res = []
    for spec, o in zip(out_specs, out):
        nested = spec.get("rlevel_max", 0) > 0 or spec.get("dlevel_max", 0) > 1
        if spec["logical_type"] == K.COL_STRING:
            vals = [v for part in o["values"] for v in part]
        elif spec["logical_type"] == K.COL_FLOAT:
            # (bit for bit: concatenated as words)
            vals = np.concatenate([np.asarray(p, np.float64).view(np.uint64) if
                                   np.asarray(p).dtype == np.float64 else np.asarray(p, np.uint64)
                                   for p in o["values"]]).view(np.float64)
        else:
            vals = np.concatenate([np.asarray(p, np.uint64) for p in o["values"]])
        r = dict(values=vals, present=None, rl=None, dl=None)
        if nested:
            r["rl"] = np.concatenate(o["rl"]).astype(np.uint64)
            r["dl"] = np.concatenate(o["dl"]).astype(np.uint64)
        elif spec.get("dlevel_max", 0):
            r["present"] = np.concatenate(o["present"]).astype(np.uint8)
        res.append(r)
    return res, rows


def expected_image(files_oldest_first, out_specs, row_order, page_order=K.PAGE_ORDER_COLUMNS,
                   filters=None):
    """the file bytes of the compacted table (column-after-column page placement: what
    E.Writer produces; the row-wise placement is the reference writer's, see
    test_gpu_chain_compact.py)"""
    if page_order != K.PAGE_ORDER_COLUMNS:
        raise NotImplementedError("E.Writer places pages column after column")
    cols, rows = expected_columns(files_oldest_first, out_specs, row_order, filters)
    w = E.Writer(out_specs)
    for spec, c in zip(out_specs, cols):
        w.put(spec["name"], c["values"], rlvl=c["rl"], dlvl=c["dl"], present=c["present"])
    w.commit(rows)
    img = w.image()
    w.close()
    return img


def oracle_chain(files_oldest_first, filters, schema, kw):
    """the rows of Plan(schema, **kw) over the partition as PartitionCursor feeds them to ONE
    GroupByExpression.  Flat scans: orc_query_run_chain.  The oracle does not restate chains
    of nested scans; for those the partial aggregates of every file (each under its filter)
    are merged, frames handed over oldest file first so that a non-aggregate select
    expression keeps the group's first row in scan order (the construction and its reason:
    test_gpu_nested_filter.oracle_chain)."""
    import oracle_lib as O
    from eventql_amd.plan import Plan
    scan = list(reversed(files_oldest_first))
    if kw.get("scan_mode", K.SCAN_FLAT) == K.SCAN_FLAT:
        return O.oracle_run_chain([f[1] for f in scan], filters, Plan(schema, **kw))
    frames = []
    for f, flt in zip(scan, filters):
        r = O.oracle_run(f[1], Plan(schema, mode=K.MODE_PARTIAL, row_filter=flt, **kw))
        keys = [r.keys[20 * i:20 * i + 20] for i in range(r.nrows)]
        frames.append(O.partial_frame(keys, r.columns[0]))
    return O.oracle_merge(Plan(schema, **kw), frames[::-1])


def lsm_columns(specs_tail=("__lsm_is_update", "__lsm_id", "__lsm_version", "__lsm_sequence")):
    U, B, S = K.COL_UNSIGNED_INT, K.COL_BOOLEAN, K.COL_STRING
    all_ = {
        "__lsm_is_update": dict(name="__lsm_is_update", logical_type=B,
                                storage_type=K.ENC_BOOLEAN_BITPACKED),
        "__lsm_id": dict(name="__lsm_id", logical_type=S, storage_type=K.ENC_STRING_PLAIN),
        "__lsm_version": dict(name="__lsm_version", logical_type=U,
                              storage_type=K.ENC_UINT64_LEB128),
        "__lsm_sequence": dict(name="__lsm_sequence", logical_type=U,
                               storage_type=K.ENC_UINT64_LEB128)}
    return [all_[n] for n in specs_tail]


def flat_out_specs():
    """the payload columns of lsm_tables + the LSM columns a compacted file keeps"""
    U, F, S = K.COL_UNSIGNED_INT, K.COL_FLOAT, K.COL_STRING
    return [
        dict(name="rid", logical_type=U, storage_type=K.ENC_UINT64_PLAIN),
        dict(name="k", logical_type=U, storage_type=K.ENC_UINT64_LEB128),
        dict(name="a", logical_type=U, storage_type=K.ENC_UINT64_PLAIN),
        dict(name="n", logical_type=U, storage_type=K.ENC_UINT64_LEB128, dlevel_max=1),
        dict(name="v", logical_type=F, storage_type=K.ENC_FLOAT_IEEE754),
        dict(name="s", logical_type=S, storage_type=K.ENC_STRING_PLAIN)] + lsm_columns()


def nested_out_specs():
    U, S = K.COL_UNSIGNED_INT, K.COL_STRING
    return [
        dict(name="id", logical_type=U, storage_type=K.ENC_UINT64_PLAIN),
        dict(name="k", logical_type=U, storage_type=K.ENC_UINT64_LEB128),
        dict(name="s", logical_type=S, storage_type=K.ENC_STRING_PLAIN),
        dict(name="items.position", logical_type=U, storage_type=K.ENC_UINT32_BITPACKED,
             rlevel_max=1, dlevel_max=2, bitpack_max_value=63),
        dict(name="items.price", logical_type=U, storage_type=K.ENC_UINT64_LEB128,
             rlevel_max=1, dlevel_max=2)] + lsm_columns()
