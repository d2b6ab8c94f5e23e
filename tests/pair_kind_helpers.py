"""Helper of the pair-arrangement tests: the leaf table the GPU layout gives a scene's BVH, restated in numpy."""


def leaf_table(bvh) -> list:
    """(start, count) of the reference tree's leaves in left-first depth-first order: the order the GPU layout numbers
    them in (include/nori_hip.h nh_bvh_node: word0 bit 0 = leaf, the rest its size; word1 = start / right child, the
    left child follows its parent)."""
    nodes, out, stack = bvh.nodes(), [], [0]
    while stack:
        i = stack.pop()
        w0, w1 = int(nodes[i][0]), int(nodes[i][1])
        if w0 & 1:
            out.append((w1, w0 >> 1))
        else:
            stack += [w1, i + 1]
    return out
