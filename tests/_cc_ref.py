"""Connected components by a plain Python union-find whose root is the smallest index: the
reference of the device clustering (hymet_mash_link / hymet_mash_labels)."""
import numpy as np


def labels(n, edges):
    """int32 [n]: for every vertex the smallest vertex of its component under `edges`."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in edges:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)], np.int32)
