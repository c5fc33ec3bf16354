from tianshou_amd.utils.statistics import (DeviceRunningMeanStd, DeviceScalarRMS, MovAvg,
                                           RunningMeanStd)

__all__ = ["MovAvg", "RunningMeanStd", "DeviceRunningMeanStd", "DeviceScalarRMS"]
