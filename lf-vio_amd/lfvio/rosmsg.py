"""ROS 1 wire format of the messages estimator_node.cpp consumes, and a minimal rosbag (format 2.0) reader / writer.

No ROS is needed: a bag recorded where the reference runs — `rosbag record /imu0 /feature_tracker/feature
/feature_tracker/restart /vins_estimator/lfvt_bootstrap` — becomes an LFVT trace (host/replay.h) through
tools/bag_to_lfvt.py.  Message layouts are the published ROS 1 serialization of
  sensor_msgs/Imu          header, orientation (4 f64) + covariance (9), angular_velocity (3) + covariance (9),
                           linear_acceleration (3) + covariance (9)                (imu_callback, estimator_node.cpp:136-161)
  sensor_msgs/PointCloud   header, points[] (u32 n, n x 3 f32), channels[] (u32 m, each: string name, f32[] values)
                           (feature_tracker_node.cpp:113-178 -> estimator_node.cpp:292-312)
  sensor_msgs/Image        header, u32 height, u32 width, string encoding, u8 is_bigendian, u32 step, u8[] data — the camera topic
                           img_callback takes (feature_tracker_node.cpp:28-78), for recordings with raw images (record type 10)
  sensor_msgs/PointCloud2  header, u32 height, u32 width, fields[] (u32 m, each: string name, u32 offset, u8 datatype, u32 count),
                           u8 is_bigendian, u32 point_step, u32 row_step, u8[] data, u8 is_dense — the lidar topic of
                           pointcloud_image_fusion (pointcloud_callback, pointcloud_image_fusion_node.cpp:121-125), for lfvio_cloud_fuse
  std_msgs/Bool            u8                                                       (restart_callback, :187-204)
  std_msgs/Float64MultiArray  layout (dim[], data_offset), f64[] data — the bootstrap record the dump hook of
                           INTEGRATION.md section 3 publishes (247 doubles + the stamp of Headers[WINDOW_SIZE])
header = u32 seq, u32 stamp.sec, u32 stamp.nsec, string frame_id; string = u32 length + bytes; little-endian throughout.
The writer exists for the tests (a synthetic bag with the layout of a real one); the reader handles uncompressed and bz2
chunks (lz4 chunks need `rosbag decompress` first).
"""
import bz2
import struct

import numpy as np


# ---------------------------------------------------------------- messages
def _string(b):
    return struct.pack("<I", len(b)) + b


def _header(seq, stamp, frame_id=b""):
    sec = int(np.floor(stamp))
    nsec = int(round((stamp - sec) * 1e9))
    if nsec >= 1000000000:
        sec, nsec = sec + 1, nsec - 1000000000
    return struct.pack("<III", seq, sec, nsec) + _string(frame_id)


def _read_header(buf, o):
    seq, sec, nsec = struct.unpack_from("<III", buf, o)
    (n,) = struct.unpack_from("<I", buf, o + 12)
    return sec + nsec * 1e-9, o + 16 + n


def ser_imu(seq, stamp, acc, gyr, frame_id=b"imu"):
    z9 = struct.pack("<9d", *([0.0] * 9))
    return (_header(seq, stamp, frame_id) + struct.pack("<4d", 0.0, 0.0, 0.0, 1.0) + z9 + struct.pack("<3d", *gyr) + z9
            + struct.pack("<3d", *acc) + z9)


def de_imu(buf):
    """-> (stamp, acc[3], gyr[3])  (header.stamp.toSec(), linear_acceleration, angular_velocity)"""
    stamp, o = _read_header(buf, 0)
    o += 8 * (4 + 9)
    gyr = struct.unpack_from("<3d", buf, o)
    o += 8 * (3 + 9)
    acc = struct.unpack_from("<3d", buf, o)
    return stamp, np.array(acc), np.array(gyr)


CHANNELS = (b"id_of_point", b"u_of_point", b"v_of_point", b"velocity_x_of_point", b"velocity_y_of_point", b"velocity_z_of_point")


def ser_pointcloud(seq, stamp, rec9, frame_id=b"world"):
    """rec9: [n, 9] float32 as an LFVT feature record holds them: point x y z, then the six channel values."""
    a = np.asarray(rec9, dtype="<f4").reshape(-1, 9)
    out = _header(seq, stamp, frame_id) + struct.pack("<I", len(a)) + a[:, 0:3].tobytes() + struct.pack("<I", 6)
    for c, name in enumerate(CHANNELS):
        out += _string(name) + struct.pack("<I", len(a)) + np.ascontiguousarray(a[:, 3 + c]).tobytes()
    return out


def de_pointcloud(buf):
    """-> (stamp, [n, 9] float32)"""
    stamp, o = _read_header(buf, 0)
    (n,) = struct.unpack_from("<I", buf, o)
    o += 4
    pts = np.frombuffer(buf, dtype="<f4", count=3 * n, offset=o).reshape(n, 3)
    o += 12 * n
    (m,) = struct.unpack_from("<I", buf, o)
    o += 4
    rec = np.zeros((n, 9), dtype="<f4")
    rec[:, 0:3] = pts
    for c in range(m):
        (ln,) = struct.unpack_from("<I", buf, o)
        o += 4 + ln
        (k,) = struct.unpack_from("<I", buf, o)
        o += 4
        if c < 6:
            assert k == n, "channel length differs from the number of points"
            rec[:, 3 + c] = np.frombuffer(buf, dtype="<f4", count=k, offset=o)
        o += 4 * k
    assert m >= 6, "the tracker publishes six channels (feature_tracker_node.cpp:152-163)"
    return stamp, rec


def ser_match_points(seq, stamp, xyid, t_q_index, frame_id=b"world"):
    """/pose_graph/match_points (sensor_msgs/PointCloud): points = (x, y, id); channels[0] = t.x t.y t.z q.w q.x q.y q.z index."""
    a = np.asarray(xyid, dtype="<f4").reshape(-1, 3)
    v = np.asarray(t_q_index, dtype="<f4").reshape(-1)
    return _header(seq, stamp, frame_id) + struct.pack("<I", len(a)) + a.tobytes() + struct.pack("<I", 1) + _string(b"") + \
        struct.pack("<I", len(v)) + v.tobytes()


def de_match_points(buf):
    """-> (stamp, frame index, relo_t[3], relo_q[4] x y z w, [K, 3] (x, y, id)) of a /pose_graph/match_points message, read as
    estimator_node.cpp:260-284 reads it (channels[0]: t, q as w x y z, index)."""
    stamp, o = _read_header(buf, 0)
    (n,) = struct.unpack_from("<I", buf, o)
    o += 4
    pts = np.frombuffer(buf, dtype="<f4", count=3 * n, offset=o).reshape(n, 3).astype(np.float64)
    o += 12 * n
    (m,) = struct.unpack_from("<I", buf, o)
    o += 4
    assert m >= 1, "match_points carries t, q and the frame index in channels[0]"
    (ln,) = struct.unpack_from("<I", buf, o)
    o += 4 + ln
    (k,) = struct.unpack_from("<I", buf, o)
    o += 4
    v = np.frombuffer(buf, dtype="<f4", count=k, offset=o).astype(np.float64)
    assert k >= 8, "channels[0] = t.x t.y t.z q.w q.x q.y q.z index"
    return stamp, int(v[7]), v[0:3].copy(), np.array([v[4], v[5], v[6], v[3]]), pts


def ser_image(seq, stamp, img, step=None, encoding=b"mono8", frame_id=b"camera"):
    """sensor_msgs/Image: header, u32 height, u32 width, string encoding, u8 is_bigendian, u32 step, u8[] data.  img [height, width]
    uint8; step: bytes per row (default width; larger: zero padding)."""
    a = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = a.shape
    step = w if step is None else int(step)
    assert step >= w
    if step != w:
        a = np.concatenate([a, np.zeros((h, step - w), np.uint8)], axis=1)
    return _header(seq, stamp, frame_id) + struct.pack("<II", h, w) + _string(encoding) + struct.pack("<BI", 0, step) + struct.pack("<I", h * step) + a.tobytes()


def de_image(buf):
    """-> (stamp, img [height, width] uint8, step, encoding) of a sensor_msgs/Image in one of the encodings img_callback takes as
    they are, mono8 and 8UC1 (feature_tracker_node.cpp:64-78); anything else raises ValueError."""
    stamp, o = _read_header(buf, 0)
    h, w = struct.unpack_from("<II", buf, o)
    (ln,) = struct.unpack_from("<I", buf, o + 8)
    enc = bytes(buf[o + 12:o + 12 + ln])
    o += 12 + ln
    _, step = struct.unpack_from("<BI", buf, o)
    (n,) = struct.unpack_from("<I", buf, o + 5)
    if enc not in (b"mono8", b"8UC1"):
        raise ValueError(f"sensor_msgs/Image encoding {enc!r}: only mono8 / 8UC1")
    if step < w or n != h * step:
        raise ValueError(f"sensor_msgs/Image: {n} bytes are not {h} rows of {step} (width {w})")
    return stamp, np.frombuffer(buf, dtype=np.uint8, count=n, offset=o + 9).reshape(h, step)[:, :w].copy(), step, enc.decode()


# the encodings cv_bridge::toCvCopy(img_msg, MONO8) makes grey of, as the codes of include/lfvio.h (LFVIO_IMG_*); mono16 becomes 7
# where the message says is_bigendian
IMAGE_CODES = {b"mono8": 0, b"8UC1": 0, b"bgr8": 2, b"rgb8": 3, b"bgra8": 4, b"rgba8": 5, b"mono16": 6}
IMAGE_BPP = {0: 1, 2: 3, 3: 3, 4: 4, 5: 4, 6: 2, 7: 2}


def ser_image_raw(seq, stamp, rows, width, encoding, is_bigendian=0, frame_id=b"camera"):
    """sensor_msgs/Image from its rows as they are: rows [height, step] uint8 (padding included), `width` pixels per row, `encoding`
    the message's string (bytes).  Nothing is checked: the tests write refused messages with it too."""
    a = np.ascontiguousarray(rows, dtype=np.uint8)
    h, step = a.shape
    return _header(seq, stamp, frame_id) + struct.pack("<II", h, width) + _string(encoding) + struct.pack("<BI", is_bigendian, step) + struct.pack("<I", h * step) + a.tobytes()


def de_image_any(buf):
    """-> (stamp, rows [height, step] uint8, width, step, code) of a sensor_msgs/Image in one of the encodings the node's cv_bridge call
    takes (feature_tracker_node.cpp:64-78): mono8, 8UC1, bgr8, rgb8, bgra8, rgba8, mono16 (IMAGE_CODES; big-endian mono16: code 7).
    The rows are the message's, padding included.  Anything else, or a step below width * bytes per pixel, raises ValueError."""
    stamp, o = _read_header(buf, 0)
    h, w = struct.unpack_from("<II", buf, o)
    (ln,) = struct.unpack_from("<I", buf, o + 8)
    enc = bytes(buf[o + 12:o + 12 + ln])
    o += 12 + ln
    big, step = struct.unpack_from("<BI", buf, o)
    (n,) = struct.unpack_from("<I", buf, o + 5)
    if enc not in IMAGE_CODES:
        raise ValueError(f"sensor_msgs/Image encoding {enc!r}: not one of {sorted(k.decode() for k in IMAGE_CODES)}")
    code = IMAGE_CODES[enc]
    if code == 6 and big:
        code = 7
    if step < w * IMAGE_BPP[code] or n != h * step:
        raise ValueError(f"sensor_msgs/Image: {n} bytes are not {h} rows of {step} (width {w}, {IMAGE_BPP[code]} bytes per pixel)")
    return stamp, np.frombuffer(buf, dtype=np.uint8, count=n, offset=o + 9).reshape(h, step).copy(), w, step, code


POINTFIELD_FLOAT32 = 7  # sensor_msgs/PointField: INT8 1, UINT8 2, INT16 3, UINT16 4, INT32 5, UINT32 6, FLOAT32 7, FLOAT64 8


def ser_pointcloud2(seq, stamp, data, fields, point_step, width, height=1, is_bigendian=0, is_dense=1, row_step=None, frame_id=b"lidar"):
    """sensor_msgs/PointCloud2 from its data bytes as they are.  fields: [(name bytes, offset, datatype, count)]; row_step: default
    width * point_step.  Nothing is checked: the tests write refused messages with it too."""
    d = np.ascontiguousarray(data, dtype=np.uint8).tobytes()
    out = _header(seq, stamp, frame_id) + struct.pack("<II", height, width) + struct.pack("<I", len(fields))
    for name, offset, datatype, count in fields:
        out += _string(name) + struct.pack("<IBI", offset, datatype, count)
    row_step = width * point_step if row_step is None else row_step
    return out + struct.pack("<BII", is_bigendian, point_step, row_step) + struct.pack("<I", len(d)) + d + struct.pack("<B", is_dense)


def de_pointcloud2(buf):
    """-> (stamp, dict(height, width, fields [(name, offset, datatype, count)], is_bigendian, point_step, row_step, data uint8 [n *
    point_step], is_dense)) of a sensor_msgs/PointCloud2 whose height * width points lie one behind the other: row_step == width *
    point_step and height * row_step data bytes.  Anything else raises ValueError."""
    stamp, o = _read_header(buf, 0)
    height, width, m = struct.unpack_from("<III", buf, o)
    o += 12
    fields = []
    for _ in range(m):
        (ln,) = struct.unpack_from("<I", buf, o)
        name = bytes(buf[o + 4:o + 4 + ln])
        offset, datatype, count = struct.unpack_from("<IBI", buf, o + 4 + ln)
        fields.append((name, offset, datatype, count))
        o += 4 + ln + 9
    big, point_step, row_step = struct.unpack_from("<BII", buf, o)
    (n,) = struct.unpack_from("<I", buf, o + 9)
    if row_step != width * point_step or n != height * row_step:
        raise ValueError(f"sensor_msgs/PointCloud2: {n} bytes in rows of {row_step} are not {height} x {width} points of {point_step} bytes")
    data = np.frombuffer(buf, dtype=np.uint8, count=n, offset=o + 13).copy()
    return stamp, dict(height=height, width=width, fields=fields, is_bigendian=big, point_step=point_step, row_step=row_step, data=data,
                       is_dense=buf[o + 13 + n])


def pointcloud2_xyz(msg):
    """(point_step, off_x, off_y, off_z, big_endian) of a de_pointcloud2 message: what lfvio_cloud_fuse takes beside the data bytes.  The
    fields named x, y and z must each be one FLOAT32; a message without one of them raises ValueError."""
    off = {}
    for name, offset, datatype, count in msg["fields"]:
        if name in (b"x", b"y", b"z"):
            if datatype != POINTFIELD_FLOAT32 or count != 1:
                raise ValueError(f"sensor_msgs/PointCloud2: field {name.decode()} is not one FLOAT32")
            off[name] = offset
    missing = [k.decode() for k in (b"x", b"y", b"z") if k not in off]
    if missing:
        raise ValueError(f"sensor_msgs/PointCloud2: no field {', '.join(missing)}")
    return msg["point_step"], off[b"x"], off[b"y"], off[b"z"], 1 if msg["is_bigendian"] else 0


def ser_bool(v):
    return struct.pack("<B", 1 if v else 0)


def de_bool(buf):
    return buf[0] != 0


def ser_f64_array(data):
    d = np.asarray(data, dtype="<f8").ravel()
    return struct.pack("<I", 0) + struct.pack("<I", 0) + struct.pack("<I", len(d)) + d.tobytes()


def de_f64_array(buf):
    (ndim,) = struct.unpack_from("<I", buf, 0)
    o = 4
    for _ in range(ndim):
        (ln,) = struct.unpack_from("<I", buf, o)
        o += 4 + ln + 8
    o += 4  # data_offset
    (n,) = struct.unpack_from("<I", buf, o)
    return np.frombuffer(buf, dtype="<f8", count=n, offset=o + 4).copy()


TYPES = {
    "sensor_msgs/Imu": "6a62c6daae103f4ff57a132d6f95cec2",
    "sensor_msgs/PointCloud": "d8e9c3f5afbdd8a130fd1d2763945fca",
    "std_msgs/Bool": "8b94c1b53db61fb6aed406028ad6332a",
    "std_msgs/Float64MultiArray": "4b7d974086d4060e7db4613a7e6c3ba4",
    "sensor_msgs/Image": "060021388200f6f0f447d0fcd9c64743",
    "sensor_msgs/PointCloud2": "1158d486dd51d683ce2f1be655c3c181",
}


# ---------------------------------------------------------------- bag container (format 2.0)
def _fields(d):
    out = b""
    for k, v in d.items():
        f = k.encode() + b"=" + v
        out += struct.pack("<I", len(f)) + f
    return out


def _record(header, data):
    h = _fields(header)
    return struct.pack("<I", len(h)) + h + struct.pack("<I", len(data)) + data


def _time(t):
    sec = int(np.floor(t))
    return struct.pack("<II", sec, int(round((t - sec) * 1e9)) % 1000000000)


class BagWriter:
    """Enough of a bag for the reader below and for `rosbag info / play`: bag header, chunks with connection + message
    records, index-less (a real recorder also writes index and chunk-info records, which readers may skip)."""

    def __init__(self, path, compression="none", chunk_messages=64):
        self.f = open(path, "wb")
        self.f.write(b"#ROSBAG V2.0\n")
        fields = {"op": b"\x03", "index_pos": struct.pack("<Q", 0), "conn_count": struct.pack("<I", 0), "chunk_count": struct.pack("<I", 0)}
        self.f.write(_record(fields, b" " * (4096 - 8 - len(_fields(fields)))))  # the bag header record is padded to 4096 bytes
        self.compression, self.per_chunk = compression, chunk_messages
        self.conns, self.buf, self.n = {}, b"", 0

    def _conn(self, topic, mtype):
        if topic in self.conns:
            return self.conns[topic]
        cid = len(self.conns)
        self.conns[topic] = cid
        data = _fields({"topic": topic.encode(), "type": mtype.encode(), "md5sum": TYPES[mtype].encode(), "message_definition": b""})
        self.buf += _record({"op": b"\x07", "conn": struct.pack("<I", cid), "topic": topic.encode()}, data)
        return cid

    def write(self, topic, mtype, t, payload):
        cid = self._conn(topic, mtype)
        self.buf += _record({"op": b"\x02", "conn": struct.pack("<I", cid), "time": _time(t)}, payload)
        self.n += 1
        if self.n % self.per_chunk == 0:
            self._flush()

    def _flush(self):
        if not self.buf:
            return
        data = bz2.compress(self.buf) if self.compression == "bz2" else self.buf
        self.f.write(_record({"op": b"\x05", "compression": self.compression.encode(), "size": struct.pack("<I", len(self.buf))}, data))
        self.buf = b""

    def close(self):
        self._flush()
        self.f.close()


def _parse_fields(h):
    out, o = {}, 0
    while o < len(h):
        (n,) = struct.unpack_from("<I", h, o)
        k, _, v = h[o + 4:o + 4 + n].partition(b"=")
        out[k.decode()] = v
        o += 4 + n
    return out


def _records(buf, o=0):
    while o + 4 <= len(buf):
        (hl,) = struct.unpack_from("<I", buf, o)
        h = _parse_fields(buf[o + 4:o + 4 + hl])
        (dl,) = struct.unpack_from("<I", buf, o + 4 + hl)
        yield h, buf[o + 8 + hl:o + 8 + hl + dl]
        o += 8 + hl + dl


def read_bag(path):
    """Yield (topic, type, receive time, payload bytes) in file order (the order the messages were received in)."""
    raw = open(path, "rb").read()
    assert raw.startswith(b"#ROSBAG V2.0\n"), "not a rosbag 2.0 file"
    conns = {}

    def walk(buf, o=0):
        for h, data in _records(buf, o):
            op = h["op"][0]
            if op == 0x03:  # bag header (its data is padding)
                continue
            if op == 0x05:
                comp = h["compression"].decode()
                if comp == "bz2":
                    data = bz2.decompress(data)
                elif comp != "none":
                    raise ValueError(f"chunk compression {comp}: run `rosbag decompress` first")
                yield from walk(data)
            elif op == 0x07:
                cid = struct.unpack("<I", h["conn"])[0]
                f = _parse_fields(data)
                conns[cid] = (h["topic"].decode(), f["type"].decode())
            elif op == 0x02:
                cid = struct.unpack("<I", h["conn"])[0]
                sec, nsec = struct.unpack("<II", h["time"])
                topic, mtype = conns[cid]
                yield topic, mtype, sec + nsec * 1e-9, data
            # 0x04 index data, 0x06 chunk info: not needed to read the messages in order

    yield from walk(raw, 13)
