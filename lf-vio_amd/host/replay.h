// replay.h — ROS-free recording of what estimator_node.cpp consumes, and the loop that feeds it to the WindowEstimator
// (SURVEY §8f rank 1).  A trace is the two topics of the node in arrival order plus what stands in for initialStructure():
//
//   file   = "LFVT" u32 version(1)  { u32 type, u32 bytes, payload[bytes] }*          (little-endian, packed)
//   type 1 = sensor_msgs/Imu          f64 stamp, f64 linear_acceleration[3], f64 angular_velocity[3]   (imu_callback, estimator_node.cpp:136-161)
//   type 2 = sensor_msgs/PointCloud   f64 stamp, u32 n, n x f32[9]:
//                                     points[i].{x,y,z} (geometry_msgs/Point32: float32 — the bearing as the tracker
//                                     published it, feature_tracker_node.cpp:146-151), then channels[0..5].values[i]:
//                                     id * NUM_OF_CAM + cam, u, v, velocity x, y, z (:152-163; decoded at estimator_node.cpp:292-312)
//   type 3 = bootstrap                f64 Ps[11][3], Rs[11][9] (row-major), Vs[11][3], Bas[11][3], Bgs[11][3], g[3], tic[3], ric[9], td
//                                     [, f64 stamp] — the window state initialStructure() + visualInitialAlign() produced
//                                     (estimator.cpp:160-173), dumped where initialStructure() returns true; the optional
//                                     stamp is Headers[WINDOW_SIZE] of that moment: the record is then used for the image
//                                     with that stamp (earlier images of a filling window slide, as after a failed
//                                     initialStructure(), :177-178), without it at the first full window.  A recording may
//                                     hold several: after failureDetection() rebooted the estimator (:196-204) or a restart
//                                     message cleared it, the next one in the file is taken.
//   type 4 = ground truth (optional)  f64 stamp, p[3], q[4] (x y z w); skipped by the replay, read by tools/ate.py
//   type 5 = restart                  [f64 stamp] — std_msgs/Bool(true) on the tracker's restart topic: restart_callback
//                                     (estimator_node.cpp:187-204) clears the buffers, clearState(), setParameter()
//
//   type 6 = relocalization           a /pose_graph/match_points message (TraceRelo below)
//   type 7 = SfM result               f64 stamp (Headers[WINDOW_SIZE] when GlobalSFM::construct() and the PnP loop had succeeded),
//                                     u32 F, F x { f64 stamp, R[9] (row-major), T[3] }: all_image_frame's R, T just before
//                                     visualInitialAlign() (estimator.cpp:358).  Handed to an initializing estimator exactly as
//                                     bootstrap records are (records that describe a time before a reboot are skipped); the
//                                     estimator aligns it with its own IMU data (WindowEstimator::visualInitialAlign).  A
//                                     bootstrap record for the same image wins.
//
//   type 8 = SfM structure            f64 stamp (Headers[WINDOW_SIZE] when GlobalSFM::construct() had succeeded), u32 K, u32 P,
//                                     K x { f64 stamp, q[4] (w x y z), T[3] }: Q[i], T[i] of the window's keyframes as construct()
//                                     returns them (estimator.cpp:268-286), P x { f64 id, xyz[3] }: sfm_tracked_points.  Handed
//                                     over as type 7 is; the estimator runs the PnP loop (estimator.cpp:288-357,
//                                     WindowEstimator::solvePnpFrames) and then the same alignment.  A bootstrap record or an
//                                     SfM result for the same image wins.
//
//   type 9 = relative pose            f64 stamp (Headers[WINDOW_SIZE] when relativePose() had returned true), i32 l, f64 R[9] (row-major),
//                                     f64 T[3]: relative_R, relative_T and l as relativePose() returns them (estimator.cpp:270-277).
//                                     Handed over as type 8 is; the estimator runs GlobalSFM::construct() on the device
//                                     (WindowEstimator::constructSfm), then the PnP loop and the same alignment.  A bootstrap
//                                     record, an SfM result or an SfM structure for the same image wins.
//
//   type 10 = sensor_msgs/Image       f64 stamp, u32 width, u32 height, u32 step, u32 encoding, then height x step bytes: a raw camera
//                                     image, for the tracker of feature_tracker.h (image_replay.h runs it over a recording and
//                                     replaces every image by what the node would have published for it).  encoding: the codes of
//                                     include/lfvio.h and csrc/image_format.h — 0 mono8 / 8UC1, 2 bgr8, 3 rgb8, 4 bgra8, 5 rgba8,
//                                     6 mono16 (little endian), 7 mono16 (big endian); the device makes grey of them.  The loader
//                                     keeps the stamp, the sizes, the code and the file offset of the pixels, not the pixels.
//                                     Refused: a record shorter or longer than its sizes say, step < width * bytes per pixel or
//                                     above 65536, a width or height outside [16, 8192], a code outside the table (1, or above 7),
//                                     images of differing size or encoding, a file that holds both type 2 and type 10.  replay()
//                                     does not look at raw images.
//
// Unknown record types are skipped, so a recorder can add its own.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "window_estimator.h"

namespace lfvio {

struct TraceImu {
  double t;
  double acc[3], gyr[3];
};
struct TraceImage {
  double t;
  std::vector<float> v;  // n x 9
  size_t size() const { return v.size() / 9; }
};
struct TraceRawImage {  // record type 10, without its pixels
  double t;
  uint32_t width, height, step;
  uint64_t offset;  // of the first pixel, from the start of the file
  uint32_t encoding;  // LFVIO_IMG_*
};
struct TraceBoot {
  WindowEstimator::Bootstrap state;
  double tic[3], ric[9], td;
  double stamp;      // NaN: take it at the first full window
  size_t at_image;   // images recorded before it
};
struct TraceRelo {  // record type 6: a /pose_graph/match_points message (estimator_node.cpp:260-284)
  double stamp;
  int index;
  double t[3], q[4];               // relo_t, relo_q [x y z w]
  std::vector<Vector3d> points;    // (x, y, id), sorted by id as the pose graph sends them
  size_t at_image;                 // images recorded before it
};
struct TraceSfm {  // record type 7
  double stamp;
  WindowEstimator::SfmResult sfm;
  size_t at_image;  // images recorded before it
};
struct TraceStructure {  // record type 8
  double stamp;
  WindowEstimator::SfmStructure st;
  size_t at_image;  // images recorded before it
};
struct TraceRelative {  // record type 9
  double stamp;
  WindowEstimator::RelativePose rel;
  size_t at_image;  // images recorded before it
};
struct Trace {
  std::vector<TraceRelative> relatives;  // in file order
  std::vector<TraceSfm> sfms;         // in file order
  std::vector<TraceStructure> structures;  // in file order
  std::vector<TraceRelo> relos;       // in file order
  std::vector<TraceImu> imu;
  std::vector<TraceImage> images;
  std::vector<TraceRawImage> raw_images;  // in file order
  std::vector<TraceBoot> boots;       // in file order
  std::vector<size_t> restarts;       // restart messages: number of images recorded before each
  bool has_bootstrap = false;         // the first bootstrap record (what a recording without reboots has)
  WindowEstimator::Bootstrap bootstrap;
  double tic[3] = {0, 0, 0}, ric[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  double td = 0;
  std::string error;
  bool load(const char *path);
  bool read(std::FILE *f);  // the same from an open stream at its start (closed by the caller)
};

struct ReplayStats {
  int images, thrown, keyframes, non_keyframes, poses, failures, last_status, iterations, restarts, bootstraps, relocalizations;
};

// feature message -> what WindowEstimator::pushImage() takes (estimator_node.cpp:292-312): feature ids ascending (the
// reference keys a std::map by id), one 8-vector x y z u v vx vy vz per id (camera 0's, the first entry of an id)
struct DecodedImage {
  std::vector<int> ids;
  std::vector<double> pts;  // n x 8
};
void decodeFeatures(const TraceImage &msg, DecodedImage *out);

// getMeasurements() + process() of estimator_node.cpp (:96-134, :206-342) over a loaded trace, single-threaded;
// after every image in NON_LINEAR state one line of the trajectory file as pubOdometry() writes it
// (utility/visualization.cpp:173-179).  Returns 0 or a negative error; `stats` may be null.
// image_ms (optional): wall-clock milliseconds of every image the loop handed over — its IMU samples and processImage(), i.e. what
// process() spends per measurement (estimator_node.cpp:206-342) — in arrival order
int replay(WindowEstimator &estimator, const Trace &trace, const char *traj_path, int max_images, ReplayStats *stats, std::vector<double> *image_ms = nullptr);

}  // namespace lfvio
