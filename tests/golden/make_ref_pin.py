"""Writes tests/golden/ref_pin.json: what the compiled reference pieces (oracle/_ref/libtf_ref.so, `make -C oracle ref`)
return on the fixed inputs of tests/test_ref_pin.py, and the marching-cubes tables as the reference's source holds them.
Data only -- results and table entries, no reference code -- so that test_ref_pin runs where neither the reference nor its
compiled library is present.  Long results are stored as SHA-256 digests of their exact bits.

    make -C oracle ref && python tests/golden/make_ref_pin.py REFERENCE_SOURCE_DIR
"""
import ctypes as C
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import test_ref_pin as T  # noqa: E402  (the inputs and the digests the test computes)


def mc_tables(src_root):
    txt = open(os.path.join(src_root, "3rd_party/open_chisel/marching_cubes/MarchingCubes.cpp")).read()
    body = txt[txt.index("triangleTable[256][16]"):]
    rows = re.findall(r"\{([^{}]*)\}", body[body.index("{") + 1:])[:256]
    tri = [[int(x) for x in r.split(",") if x.strip()] for r in rows]
    assert len(tri) == 256 and all(len(r) == 16 for r in tri)
    pairs_re = r"\{(\s*\d+\s*,\s*\d+\s*)\}"
    pairs = txt[txt.index("edgeIndexPairs[12][2]"):]
    pairs = [[int(x) for x in p.split(",")] for p in re.findall(pairs_re, pairs)[:12]]
    cm = open(os.path.join(src_root, "Structure/ChunkManager.cpp")).read()
    cm_pairs = cm[cm.index("tempEdgeIndexPairs[12][2]"):]
    cm_pairs = [[int(x) for x in p.split(",")] for p in re.findall(pairs_re, cm_pairs)[:12]]
    offs = re.search(r"cubeIndexOffsets\s*<<([^;]*);", cm).group(1)
    offs = np.array([int(x) for x in offs.split(",")]).reshape(3, 8).T.tolist()  # column k = corner k
    return {"_source": "marching_cubes/MarchingCubes.cpp triangleTable (:28-) and edgeIndexPairs (:288-); "
                       "Structure/ChunkManager.cpp tempEdgeIndexPairs and cubeIndexOffsets (:65-75)",
            "triangle_table": tri, "edge_index_pairs": pairs, "chunk_manager_edge_index_pairs": cm_pairs,
            "cube_index_offsets": offs}


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = C.CDLL(T.REF_SO)
    T.bind_ref(ref)
    out = {"_source": "oracle/_ref/libtf_ref.so (the reference's truncator, weighter, parallel_for and SparseMat compiled "
                      "unmodified, oracle/ref_shim.cpp) on the inputs of tests/test_ref_pin.py; written by "
                      "tests/golden/make_ref_pin.py.  Data only; no reference code."}
    out["truncation"] = [T.bits_digest(T._call_n(ref.tfref_truncation_n, [np.float32(p) for p in ps], T.truncation_inputs()))
                         for ps in T.PARAM_SETS]
    out["weight"] = [T.bits_digest(T._call_n(ref.tfref_weight_n, [np.float32(w)], T.weight_inputs())) for w in T.WEIGHTS]
    out["chunk_scalars"] = T.ref_chunk_scalars(ref)
    out["parallel_for"] = T.ref_parallel_for(ref)
    out["sparse_mat"] = T.sparse_mat_digests(ref, "tfref_")
    out["marching_cubes"] = mc_tables(sys.argv[1])
    path = os.path.join(ROOT, "tests", "golden", "ref_pin.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
