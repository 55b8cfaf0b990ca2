"""MI355X-native implementation of the MIPS-Fusion render-and-optimise hot path.

Host side (this package) mirrors the reference's ``model.scene_rep`` / ``model.decoder`` /
``model.encodings`` interfaces; the arithmetic runs in hand-written HIP kernels for gfx950
behind the C ABI declared in ``include/mipsf.h`` (``mipsfusion_amd/csrc``).  There is no CPU
fallback: using an operator without the built library or without a GPU raises.
"""
__version__ = "0.1.0"

_MESH = ("marching_cubes", "extract_mesh", "extract_mesh2", "Mesh", "save_ply", "load_ply")


def __getattr__(name):
    # the mesh interface (mipsfusion_amd/mesh.py), resolved on first use so that importing the package stays free of torch
    if name in _MESH:
        from . import mesh
        return getattr(mesh, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
