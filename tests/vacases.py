"""What the vertex arrays of a stream must be (dsa_batch_vertex_arrays), from the oracle's decode: one row per point, gathered
through the oracle's own point maps.  Shared by the host check and the GPU tests of the vertex arrays."""
import numpy as np


def quantisation_bits(att):
    """Bits of a quantised attribute of an oracle mesh (decoder type 2: quantisation, 3: octahedral normals), else 0."""
    return att.q_bits if att.seq_type == 2 else att.oct_bits if att.seq_type == 3 else 0


def gathered(att, values, num_points):
    """values[point_map], with the identity map of a point cloud and a row of zeros for an entry that is not in the array."""
    if len(att.point_map) == 0:
        return np.ascontiguousarray(values[:num_points])
    pm = att.point_map.astype(np.int64)
    ok = pm < len(values)
    out = np.zeros((num_points,) + values.shape[1:], values.dtype)
    out[ok] = values[pm[ok]]
    return out


def expected_rows(ref, a, fmt):
    """The rows of attribute a of oracle mesh `ref` in format "values" / "quantized": [points, stored components], or None where the
    quantized format leaves the attribute out (more than 16 bits)."""
    att = ref.attributes[a]
    if fmt == "quantized" and att.seq_type in (2, 3):
        if quantisation_bits(att) > 16:
            return None
        assert att.portable.min(initial=0) >= 0 and att.portable.max(initial=0) < 65536
        return gathered(att, att.portable.astype(np.uint16), ref.num_points)
    return gathered(att, att.values, ref.num_points)


def map_representatives(ref):
    """Per attribute the first attribute that is decoded in its order (one point map between them); 0xFF: a point cloud."""
    if ref.num_faces == 0 and all(len(a.point_map) == 0 for a in ref.attributes):
        return [0xFF] * len(ref.attributes)
    keys = ref.decoders_of_attributes()
    return [keys.index(k) for k in keys]
