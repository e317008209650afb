#pragma once
#include "../../../hr_min.h"  // test-only stand-in, see hr_min.h
