"""Partitions of NESTED event records for the record-scan tests: chains of cstable files
as tests/lsm_tables.py builds them (payload columns + __lsm_id / __lsm_is_update /
__lsm_skip / __lsm_version / __lsm_sequence), but the payload is a record with a
REPEATED RECORD items{position, price} (rlevel_max 1, dlevel_max 2) next to the
top-level columns id, k and s -- what CSTableScan reads under PartitionCursor's row
filter (server/sql/partition_cursor.cc:197-217), where the filter holds one bit per
RECORD.

A partition is a list of files OLDEST first, (file name, image, has_skiplist,
has_updates, columns dict) like lsm_tables.partition, so that
oracle_lib.oracle_partition_filters and lsm_tables.model_filters take it as it is."""
import functools

import numpy as np

import eventql_amd as E
from eventql_amd import capi as K
from lsm_tables import lsm_id

NESTED_LSM_SCHEMA = {"id": K.T_UINT64, "k": K.T_UINT64, "s": K.T_STRING,
                     "items.position": K.T_UINT64, "items.price": K.T_UINT64}

# name -> (seed, [(records, has_skiplist, has_updates)] oldest first)
PARTITIONS = {
    # updates in newer files supersede records of older ones; the middle file has a skiplist
    "basic": (201, [(3000, 0, 1), (2000, 1, 1), (2500, 0, 1)]),
    # a file of ONE record in the middle; every file long enough holds a record without
    # items and a record whose items cross the border of a 2048-slot tile (_counts)
    "edges": (202, [(2600, 0, 1), (1, 1, 1), (1800, 1, 1)]),
    # no skiplists, has_updates = false everywhere: no file gets a filter
    "quiet": (203, [(1500, 0, 0), (1000, 0, 0)]),
    "single": (204, [(2200, 1, 1)]),
    # oldest file, no skiplist, nothing remembered: scanned whole, setFilter is not called
    "single_plain": (205, [(2200, 0, 1)]),
}

def _counts(rng, nrec):
    """items per record: geometric 0..8; record 1 has none; the record that starts last in
    front of slot 2040 gets 30 items, so that its slots lie on both sides of slot 2048"""
    cnt = np.minimum(rng.geometric(0.35, nrec) - 1, 8)
    if nrec > 1:
        cnt[1] = 0
    slots = np.maximum(cnt, 1)
    starts = np.concatenate([[0], np.cumsum(slots)[:-1]])
    if starts[-1] > 2040:
        r = int(np.searchsorted(starts, 2040, side="right")) - 1
        cnt[r] = 30
    return cnt


def _file_image(rng, file_index, nrec, has_skiplist, id_space):
    who = rng.integers(0, id_space, nrec)
    upd = (rng.random(nrec) < 0.3).astype(np.uint64)
    skip = (rng.random(nrec) < 0.1).astype(np.uint64)
    i = np.arange(nrec, dtype=np.uint64)
    cnt = _counts(rng, nrec)
    slots = np.maximum(cnt, 1)  # a record without items still has one (r=0, d=0) slot
    total = int(slots.sum())
    starts = np.concatenate([[0], np.cumsum(slots)[:-1]])
    rl = np.ones(total, np.uint64)
    rl[starts] = 0
    rec_of_slot = np.repeat(np.arange(nrec), slots)
    dl = np.where(cnt[rec_of_slot] > 0, 2, 0).astype(np.uint64)
    pos = (np.arange(total) - starts[rec_of_slot] + 1).astype(np.uint64)
    price = rng.integers(1, 100000, total).astype(np.uint64)
    cols = dict(
        id=np.uint64(file_index) * np.uint64(10_000_000) + i,
        k=(who % 40).astype(np.uint64),
        s=[b"g%d" % (w % 13) if w % 7 else b"" for w in who],
        cnt=cnt, starts=starts, pos=pos, price=price, defined=dl == 2, rec_of_slot=rec_of_slot,
        ids=[lsm_id(int(w)) for w in who], upd=upd, skip=skip, who=who)
    specs = [
        dict(name="id", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
        dict(name="k", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_LEB128),
        dict(name="s", logical_type=K.COL_STRING, storage_type=K.ENC_STRING_PLAIN),
        dict(name="items.position", logical_type=K.COL_UNSIGNED_INT,
             storage_type=K.ENC_UINT32_BITPACKED, rlevel_max=1, dlevel_max=2,
             bitpack_max_value=63),
        dict(name="items.price", logical_type=K.COL_UNSIGNED_INT,
             storage_type=K.ENC_UINT64_LEB128, rlevel_max=1, dlevel_max=2),
        dict(name="__lsm_is_update", logical_type=K.COL_BOOLEAN,
             storage_type=K.ENC_BOOLEAN_BITPACKED)]
    if has_skiplist:
        specs.append(dict(name="__lsm_skip", logical_type=K.COL_BOOLEAN,
                          storage_type=K.ENC_BOOLEAN_BITPACKED))
    specs += [
        dict(name="__lsm_id", logical_type=K.COL_STRING, storage_type=K.ENC_STRING_PLAIN),
        dict(name="__lsm_version", logical_type=K.COL_UNSIGNED_INT,
             storage_type=K.ENC_UINT64_LEB128),
        dict(name="__lsm_sequence", logical_type=K.COL_UNSIGNED_INT,
             storage_type=K.ENC_UINT64_LEB128)]
    w = E.Writer(specs)
    w.put("id", cols["id"])
    w.put("k", cols["k"])
    w.put("s", cols["s"])
    w.put("items.position", pos, rlvl=rl, dlvl=dl)
    w.put("items.price", price, rlvl=rl, dlvl=dl)
    w.put("__lsm_is_update", upd)
    if has_skiplist:
        w.put("__lsm_skip", skip)
    w.put("__lsm_id", cols["ids"])
    w.put("__lsm_version", i + np.uint64(1))
    w.put("__lsm_sequence", i + np.uint64(file_index * 1_000_000 + 1))
    w.commit(nrec)
    img = w.image()
    w.close()
    return img, cols


@functools.lru_cache(maxsize=None)
def partition(name):
    """[(file name, image bytes, has_skiplist, has_updates, columns dict)], oldest first"""
    seed, files = PARTITIONS[name]
    rng = np.random.default_rng(seed)
    total = sum(f[0] for f in files)
    id_space = max(4, total // 2)
    out = []
    for fi, (nrec, skl, upd) in enumerate(files):
        img, cols = _file_image(rng, fi, nrec, bool(skl), id_space)
        out.append(("%s_%02d" % (name, fi), img, bool(skl), bool(upd), cols))
    return out
