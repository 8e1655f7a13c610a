// project_rotation.hpp -- the rotation matrix of an orientation as the reference builds it in float; shared by the
// projection kernels (prep_kernels.hpp) and their adjoint (grad_kernels.hpp), which has to land on the same pixels.
#ifndef BIOEM_PROJECT_ROTATION_HPP
#define BIOEM_PROJECT_ROTATION_HPP

namespace
{

__device__ inline void rotation_matrix(const float4 a, int isQuat, float (&rotmat)[3][3])
{
  if (isQuat)
  {
    const float q0 = a.x, q1 = a.y, q2 = a.z, q3 = a.w; // bioem.cpp:1632-1646
    rotmat[0][0] = 1 - 2 * q1 * q1 - 2 * q2 * q2;
    rotmat[1][0] = 2 * (q0 * q1 - q2 * q3);
    rotmat[2][0] = 2 * (q0 * q2 + q1 * q3);
    rotmat[0][1] = 2 * (q0 * q1 + q2 * q3);
    rotmat[1][1] = 1 - 2 * q0 * q0 - 2 * q2 * q2;
    rotmat[2][1] = 2 * (q1 * q2 - q0 * q3);
    rotmat[0][2] = 2 * (q0 * q2 - q1 * q3);
    rotmat[1][2] = 2 * (q1 * q2 + q0 * q3);
    rotmat[2][2] = 1 - 2 * q0 * q0 - 2 * q1 * q1;
  }
  else
  {
    const float alpha = a.x, beta = a.y, gam = a.z; // bioem.cpp:1653-1672
    const float ca = cosf(alpha), sa = sinf(alpha), cb = cosf(beta), sb = sinf(beta), cg = cosf(gam), sg = sinf(gam);
    rotmat[0][0] = cg * ca - cb * sa * sg;
    rotmat[0][1] = cg * sa + cb * ca * sg;
    rotmat[0][2] = sg * sb;
    rotmat[1][0] = -sg * ca - cb * sa * cg;
    rotmat[1][1] = -sg * sa + cb * ca * cg;
    rotmat[1][2] = cg * sb;
    rotmat[2][0] = sb * sa;
    rotmat[2][1] = -sb * ca;
    rotmat[2][2] = cb;
  }
}

} // namespace

#endif
