#!/usr/bin/env python3
"""rosbag -> LFVT (lf-vio_amd/host/replay.h): the one command between a recorded run of the reference and
`lfvio_host_replay` / tools/replay_stream.py / tools/ate.py — BASELINE configs[2] (PALVIO ID01) once the bag exists.

    rosbag record -O id01_topics.bag /imu0 /feature_tracker/feature /feature_tracker/restart /vins_estimator/lfvt_bootstrap \
        /pose_graph/match_points
    python tools/bag_to_lfvt.py id01_topics.bag id01.lfvt [--imu /imu0] [--truth gt.txt]

The first three topics are the node's own inputs (estimator_node.cpp:352-356); the fourth is the dump hook of
INTEGRATION.md section 3 (one std_msgs/Float64MultiArray per successful initialStructure()).  Messages are written in the
order the bag received them, contents unchanged (float32 bearings and channels stay float32).  --truth adds ground-truth
records from a `stamp x y z qx qy qz qw` text file for tools/ate.py.  /pose_graph/match_points (a pose-graph node's loop
closures, estimator_node.cpp:197-201) becomes record type 6; /vins_estimator/lfvt_sfm (the SfM hook of INTEGRATION.md section 3:
all_image_frame's stamps, R, T just before visualInitialAlign()) becomes record type 7.  No ROS installation is needed.

--image TOPIC: a bag of the CAMERA topic (sensor_msgs/Image: mono8, 8UC1, bgr8, rgb8, bgra8, rgba8 or mono16 of either byte order —
what the node's cv_bridge call takes) and the IMU, recorded without the reference's tracker: every image becomes a raw-image record
(type 10), its rows written through unchanged in their encoding, and the feature and restart topics are left out — the tracker of this library
publishes both when the recording is tracked (lfvio_host_track_trace / lfvio_host_replay_images)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd"))


def convert(bag_path, out_path, imu_topic="/imu0", feature_topic="/feature_tracker/feature", restart_topic="/feature_tracker/restart",
            bootstrap_topic="/vins_estimator/lfvt_bootstrap", truth_path=None, relo_topic="/pose_graph/match_points",
            sfm_topic="/vins_estimator/lfvt_sfm", image_topic=None):
    import numpy as np
    from lfvio import rosmsg, trace

    w = trace.TraceWriter(out_path)
    n = dict(imu=0, images=0, restarts=0, bootstraps=0, other=0)  # (+ relocalizations / sfms, when the bag has those topics)
    for topic, mtype, t, payload in rosmsg.read_bag(bag_path):
        if topic == imu_topic:
            stamp, acc, gyr = rosmsg.de_imu(payload)
            w.imu(stamp, acc, gyr)
            n["imu"] += 1
        elif image_topic and topic == image_topic:
            stamp, rows, width, step, code = rosmsg.de_image_any(payload)
            if code == 0:
                w.image(stamp, rows[:, :width], step=step)
            else:
                w.image(stamp, rows, encoding=code, width=width)
            n["raw_images"] = n.get("raw_images", 0) + 1
        elif image_topic and topic in (feature_topic, restart_topic):  # somebody else's tracker: a recording holds one or the other
            n["other"] += 1
        elif topic == feature_topic:
            stamp, rec = rosmsg.de_pointcloud(payload)
            w._rec(trace.REC_FEATURES, __import__("struct").pack("<dI", stamp, len(rec)) + rec.tobytes())
            n["images"] += 1
        elif topic == restart_topic:
            if rosmsg.de_bool(payload):
                w.restart(t)
                n["restarts"] += 1
        elif topic == bootstrap_topic:
            w.bootstrap_payload(rosmsg.de_f64_array(payload))
            n["bootstraps"] += 1
        elif topic == relo_topic:  # relo_callback, estimator_node.cpp:197-201; used in process() :260-284
            stamp, index, relo_t, relo_q, pts = rosmsg.de_match_points(payload)
            w.relo(stamp, index, relo_t, relo_q, pts)
            n["relocalizations"] = n.get("relocalizations", 0) + 1
        elif topic == sfm_topic:  # the SfM hook of INTEGRATION.md section 3: stamp, F, F x { stamp, R[9], T[3] } -> record type 7
            d = np.asarray(rosmsg.de_f64_array(payload), dtype=np.float64)
            F = int(d[1]) if d.size >= 2 else -1
            if F < 0 or d[1] != F or d.size != 2 + 13 * F:
                raise ValueError(f"{topic}: {d.size} doubles are not stamp, F, F x 13")
            body = d[2:].reshape(F, 13)
            w.sfm(d[0], body[:, 0], body[:, 1:10], body[:, 10:13])
            n["sfms"] = n.get("sfms", 0) + 1
        else:
            n["other"] += 1
    if truth_path:
        for row in np.loadtxt(truth_path).reshape(-1, 8):
            w.truth(row[0], row[1:4], row[4:8])
    w.close()
    return n


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("bag")
    ap.add_argument("out")
    ap.add_argument("--imu", default="/imu0")
    ap.add_argument("--features", default="/feature_tracker/feature")
    ap.add_argument("--restart", default="/feature_tracker/restart")
    ap.add_argument("--bootstrap", default="/vins_estimator/lfvt_bootstrap")
    ap.add_argument("--truth", default=None)
    ap.add_argument("--relo", default="/pose_graph/match_points")
    ap.add_argument("--sfm", default="/vins_estimator/lfvt_sfm")
    ap.add_argument("--image", default=None, help="camera topic: write raw-image records (type 10) instead of the feature topic")
    a = ap.parse_args()
    print(convert(a.bag, a.out, a.imu, a.features, a.restart, a.bootstrap, a.truth, a.relo, a.sfm, a.image))
