import os, sys  # noqa: E401
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import _bootstrap  # noqa: F401,E402
from millieye_amd.yolov3.utils.utils import *  # noqa: F401,F403,E402
from millieye_amd.yolov3.utils.utils import non_max_suppression  # noqa: F401,E402
