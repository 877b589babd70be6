"""The chunk plan both staging forms of the host-resident mode feed their rows by (host_stages.chunk_plan): the batch's late
rows, in slot order, cut into chunks that never span two first-use groups.  Pure Python: no GPU, no shared library."""
import pytest

from clm_gs_amd.strategies.clm_offload.host_stages import CHUNK_ROWS, chunk_plan

CASES = [
    ([0, 0, 0, 0], 2),                       # nothing to stage: four empty chunks
    ([5, 0, 3, 0], 2),                       # no multiple of the chunk / a group without rows between two with rows
    ([4, 0, 3, 0], 2),                       # an exact multiple
    ([4, 5], 4),                             # exactly one chunk / one chunk and one row
    ([CHUNK_ROWS, CHUNK_ROWS + 1], None),    # the same at the product's chunk size
]


@pytest.mark.parametrize("n_first,chunk_rows", CASES)
def test_chunk_plan_tiles_the_rows_group_by_group(n_first, chunk_rows):
    chunks = chunk_plan(n_first) if chunk_rows is None else chunk_plan(n_first, chunk_rows)
    chunk_rows = chunk_rows or CHUNK_ROWS
    # the chunks tile [0, sum(n_first)) without gap or overlap, in order, group after group
    pos, groups = 0, []
    for i, c0, c1, first, last, g0 in chunks:
        assert c0 == pos and c0 <= c1 <= c0 + chunk_rows
        assert c1 > c0 or n_first[i] == 0    # an empty chunk only for a group without rows
        pos = c1
        groups.append(i)
    assert pos == sum(n_first)
    assert groups == sorted(groups) and sorted(set(groups)) == list(range(len(n_first)))
    start = 0
    for i, n in enumerate(n_first):
        mine = [c for c in chunks if c[0] == i]
        # every group has exactly one first and one last chunk: its first and its last
        assert [c[3] for c in mine] == [True] + [False] * (len(mine) - 1)
        assert [c[4] for c in mine] == [False] * (len(mine) - 1) + [True]
        assert len(mine) == max(1, -(-n // chunk_rows))
        # group_start is the prefix sum, and the group's chunks cover exactly its rows
        assert all(c[5] == start for c in mine)
        assert mine[0][1] == start and mine[-1][2] == start + n
        start += n


def test_all_empty_groups_are_each_first_and_last():
    assert chunk_plan([0, 0, 0, 0], 2) == [(i, 0, 0, True, True, 0) for i in range(4)]
