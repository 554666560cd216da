"""Shapes of the batched Gram tests (test infrastructure, no GPU needed): per branch of the batched plan the smallest
token lists that reach it, checked against ``qt_xtx_batched_plan`` itself before a test launches anything."""
from tests.exact_inputs import NUM_CU

# name -> (token counts, K, branch): what the plan must look like is asserted by check_branch()
CASES = {
    "all_direct": ([128, 192], 512, "every (problem, tile) pair one item added into G"),
    "all_direct_k520": ([190, 130], 520, "all direct; two ragged tails; K = 520: a ragged last tile row of 8 channels"),
    "all_slabbed": ([8192, 8192], 512, "every pair cut into chunks of 4 token tiles: slabs + table-driven reduction"),
    "mixed": ([4096, 4160, 130], 512, "long problems slabbed, the short ragged one direct, in one launch"),
    "zero_in_the_middle": ([200, 0, 1000, 64], 1024, "a zero-token problem between others; ragged tails; mixed"),
    "ragged_tails_k520": ([700, 0, 333, 64, 1000], 520, "three ragged tails, K = 520, a zero-token problem; mixed"),
    "over_256_items": ([2048] * 9, 1024, "720 items: the grid wraps the 256-block rounds of xtx_logical"),
    # beyond K = 1024 on purpose: whole rounds of direct pairs need 256 pairs, i.e. 13 problems of 21 tiles
    "whole_rounds": ([8192] + [256, 64, 200] * 4, 1536, "256 pairs in a direct round, the long problem cut to the "
                                                         "makespan cap, the pairs after the round chunked"),
}


def check_branch(name, items, n_slabs):
    """The plan of CASES[name] has the shape its branch text says (a planner change that moves a case off its branch
    fails here, not silently)."""
    tokens, K, _ = CASES[name]
    direct = [it for it in items if it[5] < 0]
    slabbed = [it for it in items if it[5] >= 0]
    assert len(slabbed) == n_slabs
    probs = {it[0] for it in items}
    assert probs == {p for p, t in enumerate(tokens) if t > 0}
    if name.startswith("all_direct"):
        assert not slabbed
    elif name == "all_slabbed":
        assert not direct and all(it[4] == 4 for it in items)
    elif name == "over_256_items":
        assert len(items) > 2 * NUM_CU and len(items) % NUM_CU != 0
    elif name == "whole_rounds":
        nt = (K + 255) // 256
        assert len(tokens) * nt * (nt + 1) // 2 >= NUM_CU
        assert any(it[0] == 0 for it in slabbed) and direct and len(items) > NUM_CU
    else:
        assert direct and slabbed
        if name == "mixed":         # the short problem whole, the long ones in chunks
            assert {it[0] for it in direct} == {2} and {it[0] for it in slabbed} == {0, 1}
