// empty but for the containers (linemod_if.h includes it); see opencv2/core.hpp
#include "opencv2/core.hpp"
