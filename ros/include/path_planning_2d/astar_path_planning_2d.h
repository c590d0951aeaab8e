// A* node class of the catkin package, rebuilt on libpp2_hip.so.
//
// Replaces include/path_planning_2d/astar_path_planning_2d.h of the reference
// (class at :27-67).  Same public interface, parameters and topics; the
// per-message jps3d search becomes one goal-rooted shortest-path field of the
// map (pp2_path_solve, include/pp2.h "shortest-path field"), solved once at
// start-up, whose action table the belief callback looks up at the belief's
// mode.  No jps3d, no Eigen.  Syntax-checked with the adapter
// (tests/test_path_cpu.py); see ros/README.md.
#ifndef ASTAR_PATH_PLANNING_2D_H
#define ASTAR_PATH_PLANNING_2D_H

#include <vector>

#include <pp2.h>

#include "path_planning_2d_base.h"

namespace path_planning_2d {

class AStarPathPlanning2d : public PathPlanning2dBase {
 public:
  typedef boost::shared_ptr<AStarPathPlanning2d> Ptr;
  typedef boost::shared_ptr<const AStarPathPlanning2d> ConstPtr;

  explicit AStarPathPlanning2d(ros::NodeHandle& n);
  AStarPathPlanning2d(const AStarPathPlanning2d&) = delete;
  AStarPathPlanning2d operator=(const AStarPathPlanning2d&) = delete;
  ~AStarPathPlanning2d();

  virtual bool initialize();

 private:
  virtual bool loadParameters();
  virtual bool createRosIO();
  virtual void beliefCallback(const dummy_simulator::BeliefConstPtr& belief);
  virtual void loadMapFromFile();

  pp2_ctx* ctx_ = nullptr;            // the map and its shortest-path field on the GPU
  std::vector<uint8_t> path_action_;  // A_path, one action per cell
};

typedef AStarPathPlanning2d::Ptr AStarPathPlanning2dPtr;
typedef AStarPathPlanning2d::ConstPtr AStarPathPlanning2dConstPtr;
}  // namespace path_planning_2d

#endif
