#pragma once
#include "../../../he_min.h"  // test-only stand-in, see he_min.h
