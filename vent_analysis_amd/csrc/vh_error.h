// The one exception type of libventhip: a status code of include/vent_hip.h and the message that
// vh_last_error() hands out.  Standard headers only; api.hip turns it into the status at the ABI.
#pragma once
#include <string>

#include "../../include/vent_hip.h"

struct VhError {
    int code;
    std::string msg;
};
