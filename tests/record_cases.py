"""Record lists for the search by which every tile kernel finds its record (afg::last_at_or_before, csrc/afg_records.h):
record counts of 1, 2 and 5 -- one, two and a count that is no power of two -- with records that have no tiles as the
first, a middle and the last record, and lengths from {0, 1, tile - 1, tile, tile + 1}.  Each stage's test_*_gpu.py runs
them through one launch each, against its own model."""


def record_lengths(tile):
    """name -> the lengths of a launch's records, in units of which `tile` make one tile"""
    return {
        "1": [tile + 1],
        "2-none-first": [0, tile],
        "2-none-last": [tile - 1, 0],
        "5-none-first-middle-last": [0, 1, 0, tile + 1, 0],
        "5": [tile, 1, 0, tile - 1, tile + 1],
    }


RECORD_CASES = list(record_lengths(2))
