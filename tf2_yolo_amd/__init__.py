"""MI355X-native YOLO training / detection path.

The package leaves GPU_MAX_HW_QUEUES (how many hardware queues the ROCm runtime maps a process's HIP streams onto) to the
environment. The training step's streams get queues of their own by being created first (ops.create_side_streams);
DESIGN.md Appendix A.4 has the measurements.
"""
