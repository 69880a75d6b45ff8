"""What the GPU tests of the resampling passes share (test_gpu_contacts.py, test_gpu_absorb.py, test_gpu_lift.py): the two
builds of the kernel library, a destination between poisoned guards, and the upload of a host volume."""
import numpy as np

from tests.parity_util import to_dev

POISON = 0xA5
GUARD = 64   # floats of poison before and behind each destination array
_libs = {}


def lib_for(variant):
    from emfusion_amd import _lib
    if variant not in _libs:
        _libs[variant] = _lib.load() if variant == "" else _lib.load_variant(variant)
    return _libs[variant]


class Guarded:
    """A destination array between two poisoned guards."""

    def __init__(self, host):
        from emfusion_amd.devmem import DeviceArray, DeviceView
        self.n = host.size
        self.buf = DeviceArray((self.n + 2 * GUARD,), np.float32).fill_bytes_(POISON)
        self.view = DeviceView(self.buf.ptr + 4 * GUARD, host.shape, np.float32)
        self.view.copy_from(host)

    def read(self):
        raw = self.buf.numpy()
        assert (raw[:GUARD].view(np.uint8) == POISON).all() and (raw[GUARD + self.n:].view(np.uint8) == POISON).all(), \
            "written outside the destination"
        return raw[GUARD:GUARD + self.n].reshape(self.view.shape)


def upload_src(src, with_map):
    """The device volume of a host one (tsdf, weights, fg or None, voxel_size, truncdist where it has one), with its
    unseen-tile map on request."""
    from emfusion_amd import ops
    from emfusion_amd.devmem import DeviceArray
    d = dict(tsdf=to_dev(src["tsdf"]), weights=to_dev(src["weights"]), voxel_size=src["voxel_size"],
             fg_mask=None if src["fg"] is None else to_dev(src["fg"]))
    if "truncdist" in src:
        d["truncdist"] = src["truncdist"]
    nz, ny, nx = src["tsdf"].shape
    if with_map and min(nx, ny, nz) >= 2:  # the map's builder takes no thinner volume
        tiles = DeviceArray((ops.unseen_tile_bytes((nx, ny, nz)),), np.uint8).fill_bytes_(POISON)
        ops.rebuild_unseen_tiles(d["tsdf"], d["weights"], tiles)
        d["unseen_tiles"] = tiles
    return d
