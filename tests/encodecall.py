"""One way for the tests and tools to reach an encode entry point of the library directly: "call entry `name` with these meshes,
options and grids; the call's status and, per mesh, (status, bytes or message)".  The native arrays are the package's own
(draco_sharp_amd.encoder._native_meshes), in the form the entry takes."""
import ctypes as C

from draco_sharp_amd import native
from draco_sharp_amd.encoder import _native_meshes

# the entries that do not take dsa_mesh_attr_input, and the ones with a dsa_mesh_grids array behind the meshes
FORMS = {"dsa_encode_batch": native.MeshInput, "dsa_encode_sequential_batch": native.MeshInput,
         "dsa_encode_batch_corners": native.MeshCornerInput, "dsa_encode_batch_ex": native.MeshCornerInput}
GRIDDED = ("dsa_encode_grid_batch", "dsa_encode_seam_repair_batch", "dsa_encode_grid_sequential_batch")
FROM_MESHES = object()


def streams(ctx, h, n, messages=True):
    """[(status, bytes, or the refusal's text / None)] of a dsa_encoded, which is freed."""
    L = native.lib()
    out = []
    p, ln = C.c_void_p(), C.c_size_t()
    for i in range(n):
        s = L.dsa_encoded_stream(h, i, C.byref(p), C.byref(ln))
        out.append((s, C.string_at(p, ln.value) if s == 0 else (ctx.error() if messages else None)))
    L.dsa_encoded_free(h)
    return out


def arrays(meshes, form=None):
    """(array of `form` or dsa_mesh_attr_input, dsa_mesh_grids array or None, keep-alive list) of MeshData / PointCloudData"""
    return _native_meshes(meshes, form)


def call(ctx, name, meshes, opt, grids=FROM_MESHES, form=None, edit=None, messages=True):
    """(call status, [(status, bytes or message) per mesh] or None).  opt: the entry's option struct or None; grids (entries that
    take them): a dsa_mesh_grids array or None, by default what the meshes themselves set; form: the struct type of the mesh
    array, by default the entry's own; edit(arr, keep): changes to the native array before the call."""
    n = len(meshes)
    arr, own_grids, keep = arrays(meshes, form or FORMS.get(name))
    if edit:
        edit(arr, keep)
    args = [ctx._h, n, arr]
    if name in GRIDDED:
        args.append(own_grids if grids is FROM_MESHES else grids)
    h = C.c_void_p()
    st = getattr(native.lib(), name)(*args, C.byref(opt) if opt is not None else None, C.byref(h))
    return st, (streams(ctx, h, n, messages) if st == 0 else None)
