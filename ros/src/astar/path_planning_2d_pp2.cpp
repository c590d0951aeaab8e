// AStarPathPlanning2d on libpp2_hip.so: replaces src/astar/path_planning_2d.cpp
// of the reference (class body :34-187) in the catkin package, together with
// the drop-in header ros/include/path_planning_2d/astar_path_planning_2d.h.
// Node main, launch file, parameters and the ~belief / ~control topics are
// unchanged.  The reference searches a path from the belief's mode to the goal
// on every message and publishes its first step; here the goal-rooted
// shortest-path field is solved once at start-up (pp2_path_solve: the first
// step of a shortest 8-connected path for every cell at once) and a message
// costs one table lookup.  Among equal-cost paths the field takes the lowest
// action number (include/pp2.h); jps3d's choice there is not pinned
// (DESIGN.md §2.3).
//
// Syntax-checked here (tests/test_path_cpu.py, stand-in ROS / OpenCV headers
// in tests/ros_stubs/); no ROS / OpenCV in the image to link it.
#include <cstdio>
#include <cstdlib>

#include <opencv2/core/core.hpp>
#include <opencv2/highgui/highgui.hpp>

#include <std_msgs/Byte.h>

#include <path_planning_2d/astar_path_planning_2d.h>

namespace path_planning_2d {

namespace {

bool pp2_ok(int status, const char* what) {
  if (status == PP2_OK) return true;
  ROS_ERROR("%s failed (%s): %s", what, pp2_status_string(status), pp2_last_error());
  return false;
}

}  // namespace

AStarPathPlanning2d::AStarPathPlanning2d(ros::NodeHandle& n) : PathPlanning2dBase(n) {}

AStarPathPlanning2d::~AStarPathPlanning2d() {
  if (ctx_) pp2_destroy(ctx_);
  ctx_ = nullptr;
  free(grid_map);
  if (planning_time_fid) fclose(planning_time_fid);
}

bool AStarPathPlanning2d::loadParameters() {
  const bool ok = nh.getParam("map_path", map_path) && nh.getParam("goal_x", goal[0]) &&
                  nh.getParam("goal_y", goal[1]) &&
                  nh.getParam("discount_factor", discount_factor) &&
                  nh.getParam("map_resolution", map_resolution);
  nh.param<std::string>("fixed_frame_id", fixed_frame_id, "map");
  nh.param<std::string>("robot_frame_id", robot_frame_id, "robot");
  return ok;
}

// 1 where the grey level is <= 250 (the reference's THRESH_BINARY_INV at 250).
void AStarPathPlanning2d::loadMapFromFile() {
  const cv::Mat img = cv::imread(map_path, cv::IMREAD_GRAYSCALE);
  map_height = img.rows;
  map_width = img.cols;
  grid_map = static_cast<uint8_t*>(malloc((size_t)map_height * map_width));
  for (uint32_t y = 0; y < map_height; ++y) {
    const uint8_t* row = img.ptr<uint8_t>(y);
    for (uint32_t x = 0; x < map_width; ++x) grid_map[(size_t)y * map_width + x] = row[x] <= 250;
  }
}

bool AStarPathPlanning2d::initialize() {
  if (!loadParameters()) {
    ROS_WARN("Cannot load all required parameters...");
    return false;
  }
  loadMapFromFile();
  if (grid_map[(size_t)goal[1] * map_width + goal[0]]) {
    ROS_ERROR("The assigned goal (%d %d) is at a occupied cell...", goal[0], goal[1]);
    return false;
  }
  if (!pp2_ok(pp2_create(&ctx_, /*device=*/0, map_height, map_width, grid_map, goal[0], goal[1],
                         discount_factor),
              "pp2_create"))
    return false;
  const size_t hw = (size_t)map_height * map_width;
  int rounds = 0, converged = 0, reached = 0;
  const ros::Time t0 = ros::Time::now();
  if (!pp2_ok(pp2_path_solve(ctx_, /*max_rounds=*/(int)hw, &rounds, &converged, &reached),
              "shortest-path field"))
    return false;
  if (!converged) {
    ROS_ERROR("The shortest-path field did not settle in %d rounds...", rounds);
    return false;
  }
  std::printf("shortest-path field: %d rounds, %d cells reach the goal, %f s\n", rounds, reached,
              (ros::Time::now() - t0).toSec());
  path_action_.resize(hw);
  if (!pp2_ok(pp2_path_get(ctx_, nullptr, path_action_.data()), "downloading the action table"))
    return false;
  if (!createRosIO()) {
    ROS_WARN("Cannot load all ROS I/O...");
    return false;
  }
  planning_time_fid = fopen("planning_time", "a+");
  return true;
}

bool AStarPathPlanning2d::createRosIO() {
  control_pub = nh.advertise<std_msgs::Byte>("control", 1);
  belief_sub = nh.subscribe("belief", 1, &AStarPathPlanning2d::beliefCallback, this);
  return true;
}

// The first step of the shortest path from the belief's mode (first maximum
// above 0; cell 0 otherwise): 4, stay, at the goal and where no path exists.
void AStarPathPlanning2d::beliefCallback(const dummy_simulator::BeliefConstPtr& msg) {
  float best = 0.0f;
  size_t mode = 0;
  for (size_t i = 0; i < msg->belief.size(); ++i)
    if (msg->belief[i] > best) best = msg->belief[mode = i];
  std_msgs::Byte out;
  out.data = mode < path_action_.size() ? path_action_[mode] : 4;
  control_pub.publish(out);
}

}  // namespace path_planning_2d
