"""CPU tests of sensor_msgs/PointCloud2 in lfvio/rosmsg.py: what lfvio_cloud_fuse's cloud arrives as.

  1  ser_pointcloud2 / de_pointcloud2 round trip, field table and data bytes as they are; the md5 in rosmsg.TYPES
  2  pointcloud2_xyz on an Ouster-like 48-byte layout, a packed 12-byte one and a Velodyne-like 22-byte one (unaligned), in both byte
     orders: the offsets it returns read the points back through fuse_ref.fields
  3  refusals: no z, a FLOAT64 x, a count of 2, rows with padding (row_step != width * point_step), a short data array"""
import numpy as np
import pytest

import fuse_ref as fr
from lfvio import rosmsg

F32, U16, U32, U8 = rosmsg.POINTFIELD_FLOAT32, 4, 6, 2
OUSTER = [(b"x", 0, F32, 1), (b"y", 4, F32, 1), (b"z", 8, F32, 1), (b"intensity", 16, F32, 1), (b"t", 20, U32, 1), (b"reflectivity", 24, U16, 1),
          (b"ring", 26, U16, 1), (b"ambient", 28, U16, 1), (b"range", 32, U32, 1)]
PACKED = [(b"x", 0, F32, 1), (b"y", 4, F32, 1), (b"z", 8, F32, 1)]
VELODYNE = [(b"ring", 0, U16, 1), (b"x", 2, F32, 1), (b"y", 6, F32, 1), (b"z", 10, F32, 1), (b"intensity", 14, F32, 1), (b"time", 18, F32, 1)]
LAYOUTS = (("ouster", OUSTER, 48), ("packed", PACKED, 12), ("velodyne", VELODYNE, 22))


def offsets(fields):
    d = {name: off for name, off, _, _ in fields}
    return d[b"x"], d[b"y"], d[b"z"]


def test_round_trip():
    assert rosmsg.TYPES["sensor_msgs/PointCloud2"] == "1158d486dd51d683ce2f1be655c3c181"
    P = fr.sphere_cloud(64 * 3, seed=3)
    data = fr.pack_cloud(P, 48, offsets(OUSTER), seed=1)
    buf = rosmsg.ser_pointcloud2(7, 12.25, data, OUSTER, 48, width=64, height=3, is_dense=0, frame_id=b"os_sensor")
    stamp, msg = rosmsg.de_pointcloud2(buf)
    assert stamp == 12.25 and (msg["height"], msg["width"], msg["point_step"], msg["row_step"]) == (3, 64, 48, 64 * 48)
    assert msg["fields"] == OUSTER and msg["is_bigendian"] == 0 and msg["is_dense"] == 0
    assert msg["data"].dtype == np.uint8 and np.array_equal(msg["data"], data)
    assert rosmsg.ser_pointcloud2(7, 12.25, msg["data"], msg["fields"], 48, width=64, height=3, is_dense=0, frame_id=b"os_sensor") == buf
    # an empty cloud
    _, empty = rosmsg.de_pointcloud2(rosmsg.ser_pointcloud2(0, 0.0, np.zeros(0, np.uint8), PACKED, 12, width=0))
    assert len(empty["data"]) == 0 and rosmsg.pointcloud2_xyz(empty) == (12, 0, 4, 8, 0)


@pytest.mark.parametrize("name,fields,step", LAYOUTS)
@pytest.mark.parametrize("big", [0, 1])
def test_field_helper(name, fields, step, big):
    P = fr.sphere_cloud(100, seed=4)
    offs = offsets(fields)
    data = fr.pack_cloud(P, step, offs, big_endian=big, seed=2)
    _, msg = rosmsg.de_pointcloud2(rosmsg.ser_pointcloud2(1, 1.0, data, fields, step, width=100, is_bigendian=big))
    got = rosmsg.pointcloud2_xyz(msg)
    assert got == (step, *offs, big)
    x, y, z = fr.fields(msg["data"], 100, *got)
    assert np.array_equal(np.stack([x, y, z], axis=1), P)
    assert not fr.check(n=100, point_step=got[0], offs=got[1:4], big_endian=got[4])


def test_refusals():
    data = fr.pack_cloud(fr.sphere_cloud(8), 12)
    de = lambda **kw: rosmsg.de_pointcloud2(rosmsg.ser_pointcloud2(1, 1.0, data, kw.pop("fields", PACKED), 12, **kw))[1]
    assert rosmsg.pointcloud2_xyz(de(width=8)) == (12, 0, 4, 8, 0)
    for fields in (PACKED[:2], [PACKED[0], PACKED[1], (b"Z", 8, F32, 1)], [(b"x", 0, 8, 1)] + PACKED[1:], [PACKED[0], (b"y", 4, F32, 2), PACKED[2]]):
        with pytest.raises(ValueError):
            rosmsg.pointcloud2_xyz(de(width=8, fields=fields))
    for kw in (dict(width=8, row_step=100), dict(width=4, height=2, row_step=96), dict(width=9), dict(width=4, height=3)):
        with pytest.raises(ValueError):
            de(**kw)
    assert len(de(width=4, height=2)["data"]) == 96
