#pragma once
#include "../../cam_min.h"  // test-only stand-in, see cam_min.h
