"""`make_pairs` and `find_closest_date_idx` with the behaviour of the reference's `post_processing/utils.py`, quirks included
(tests/golden/g17_dod.npz pins both against the reference's own run)."""
from datetime import datetime, timedelta
from pathlib import Path
from typing import List


def find_closest_date_idx(datetime_list: List[datetime], date_to_find: datetime) -> int:
    """The position of the date closest to `date_to_find`; among equally close dates, and among equal dates, the first."""
    return min(range(len(datetime_list)), key=lambda k: abs(datetime_list[k] - date_to_find))


def make_pairs(pcd_list: List[Path], step: int = 1, date_format: str = "%Y_%m_%d"):
    """({i: (path_i, path of the cloud closest to date_i + step days)}, dates) for a list of cloud paths whose stems end in a date.
    Three things are the reference's and are kept: the date of EVERY stem starts where "202" starts in the FIRST stem; the last `step`
    clouds start no pair, whatever their dates; the closest date wins even when it is the cloud's own (a gap in the series)."""
    paths = [Path(p) for p in pcd_list]
    cut = paths[0].stem.find("202")
    dates = [datetime.strptime(p.stem[cut:], date_format) for p in paths]
    ahead = timedelta(days=step)
    pairs = {}
    for first in range(len(paths) - step):
        second = find_closest_date_idx(dates, dates[first] + ahead)
        pairs[first] = (str(paths[first]), str(paths[second]))
    return pairs, dates
