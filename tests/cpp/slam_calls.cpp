// Front-end check (g++ -fsyntax-only) of the drop-in claim: every call slam.cpp makes on KalmanFilter and FeatureDetector, in the
// forms it makes them, against compat/ at the include names slam.cpp uses (tests/test_compat.py maps those names onto compat/ and
// the two stand-ins).  Nothing here is built or run.
#include <cmath>
#include <fstream>
#include <iostream>
#include <vector>

#include <Eigen/Dense>
#include "Aria.h"
#include "odometry/kalmanfilter.h"
#include "features/featuredetector.h"

void slam_calls(ArRobot &robot, ArSick &laser, std::ofstream &cov, std::ofstream &known, std::ofstream &points) {
    FeatureDetector *detector = new FeatureDetector(&laser);  // slam.cpp:110
    KalmanFilter *filter = new KalmanFilter(&robot);          // slam.cpp:127
    filter->doPropagation(0.001, cov, known);                 // slam.cpp:136
    std::vector<Feature> found;
    double heading;
    detector->getFeatures(&found, &heading, filter->Phi);     // slam.cpp:141
    if (heading != detector->NO_COMPASS)                      // slam.cpp:144-146
        filter->doUpdateCompass(heading, 0.0005);
    for (size_t k = 0; k < found.size(); k++) {               // slam.cpp:150-178
        const double px = found[k].x / 1000.0, py = found[k].y / 1000.0;
        const double range = std::sqrt(px * px + py * py), angle = std::atan2(py, px);
        Eigen::MatrixXd z(2, 1), noise(2, 2), J(2, 2), Rz(2, 2);
        z << px, py;
        noise << 0.0025, 0, 0, 0.0001;
        J << std::cos(angle), -range * std::sin(angle), std::sin(angle), range * std::cos(angle);
        Rz = J * noise * J.transpose();
        filter->doUpdate(z, Rz);                              // slam.cpp:170
        std::cout << filter->Num_Landmarks << std::endl;       // slam.cpp:171
        points << px * std::cos(filter->Phi) - py * std::sin(filter->Phi) + filter->X << " "
               << px * std::sin(filter->Phi) + py * std::cos(filter->Phi) + filter->Y << std::endl;  // slam.cpp:173-177
    }
    points << filter->X << " " << filter->Y << std::endl;      // slam.cpp:181
    delete filter;
    delete detector;
}
