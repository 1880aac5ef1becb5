! Capture wrapper for tests/golden/make_golden_coupling.py: bind(C) routines that call the reference's scale_fluxes on
! arrays handed in, set the module arrays its ocean_mixed_layer reads and call it, and call its atmo_boundary_layer for
! the 'ocn' surface on one block (for delt, delq, shcoef, lhcoef, which ocean_mixed_layer keeps in local arrays).
! Compiled against the module files of the reference build (oracle/build_ref.sh, configuration small, or gx1 for --time);
! nothing of it is committed but this text.  albocn, cprho, Lvap are parameters of ice_constants and are not set here.
      module coupling_capture
      use iso_c_binding
      use ice_kinds_mod
      use ice_domain_size
      use ice_blocks, only: nx_block, ny_block
      implicit none
      contains

      subroutine cpcap_scale (a_tmask, a_aice, a_Tf, a_Tair, a_Qa, a_strairxT, a_strairyT, a_fsens, a_flat, a_fswabs, &
                 a_flwout, a_evap, a_Tref, a_Qref, a_fresh, a_fsalt, a_fhocn, a_fswthru, a_alvdr, a_alidr, a_alvdf, &
                 a_alidf) bind(C, name='cpcap_scale')
      use ice_flux, only: scale_fluxes
      integer(c_int) :: a_tmask(nx_block,ny_block)
      real(c_double), dimension(nx_block,ny_block) :: a_aice, a_Tf, a_Tair, a_Qa, a_strairxT, a_strairyT, a_fsens, &
         a_flat, a_fswabs, a_flwout, a_evap, a_Tref, a_Qref, a_fresh, a_fsalt, a_fhocn, a_fswthru, a_alvdr, a_alidr, &
         a_alvdf, a_alidf
      logical(log_kind) :: mask(nx_block,ny_block)
      mask(:,:) = a_tmask(:,:) /= 0
      call scale_fluxes (nx_block, ny_block, mask, a_aice, a_Tf, a_Tair, a_Qa, a_strairxT, a_strairyT, a_fsens, a_flat, &
                         a_fswabs, a_flwout, a_evap, a_Tref, a_Qref, a_fresh, a_fsalt, a_fhocn, a_fswthru, a_alvdr, &
                         a_alidr, a_alvdf, a_alidf)
      end subroutine cpcap_scale

      ! ocean_mixed_layer(dt) on nb blocks: in(:,:,:,k), k = 1..17 are potT, uatm, vatm, wind, zlvl, Qa, rhoa, flw, hmix, Tf,
      ! aice, fhocn, fswthru, swvdr, swvdf, swidr, swidf; io(:,:,:,1:2) sst, qdp; out(:,:,:,k), k = 1..13 frzmlt, flwout_ocn,
      ! fsens_ocn, flat_ocn, evap_ocn, strairx_ocn, strairy_ocn, Tref_ocn, Qref_ocn, alvdr_ocn, alidr_ocn, alvdf_ocn,
      ! alidf_ocn.  Every output starts as the caller's poison.
      subroutine cpcap_mixed (nb, a_dt, a_tmask, a_in, a_io, a_out) bind(C, name='cpcap_mixed')
      use ice_flux
      use ice_state, only: aice
      use ice_grid, only: tmask
      use ice_domain, only: nblocks
      use ice_atmo, only: atmbndy, calc_strair
      use ice_ocean, only: ocean_mixed_layer
      integer(c_int), value :: nb
      real(c_double), value :: a_dt
      integer(c_int) :: a_tmask(nx_block,ny_block,nb)
      real(c_double) :: a_in(nx_block,ny_block,nb,17), a_io(nx_block,ny_block,nb,2), a_out(nx_block,ny_block,nb,13)
      integer :: b
      nblocks = nb
      atmbndy = 'default'
      calc_strair = .true.
      do b = 1, nb
         tmask(:,:,b) = a_tmask(:,:,b) /= 0
         potT(:,:,b) = a_in(:,:,b,1)
         uatm(:,:,b) = a_in(:,:,b,2)
         vatm(:,:,b) = a_in(:,:,b,3)
         wind(:,:,b) = a_in(:,:,b,4)
         zlvl(:,:,b) = a_in(:,:,b,5)
         Qa(:,:,b) = a_in(:,:,b,6)
         rhoa(:,:,b) = a_in(:,:,b,7)
         flw(:,:,b) = a_in(:,:,b,8)
         hmix(:,:,b) = a_in(:,:,b,9)
         Tf(:,:,b) = a_in(:,:,b,10)
         aice(:,:,b) = a_in(:,:,b,11)
         fhocn(:,:,b) = a_in(:,:,b,12)
         fswthru(:,:,b) = a_in(:,:,b,13)
         swvdr(:,:,b) = a_in(:,:,b,14)
         swvdf(:,:,b) = a_in(:,:,b,15)
         swidr(:,:,b) = a_in(:,:,b,16)
         swidf(:,:,b) = a_in(:,:,b,17)
         sst(:,:,b) = a_io(:,:,b,1)
         qdp(:,:,b) = a_io(:,:,b,2)
         frzmlt(:,:,b) = a_out(:,:,b,1)
         flwout_ocn(:,:,b) = a_out(:,:,b,2)
         fsens_ocn(:,:,b) = a_out(:,:,b,3)
         flat_ocn(:,:,b) = a_out(:,:,b,4)
         evap_ocn(:,:,b) = a_out(:,:,b,5)
         strairx_ocn(:,:,b) = a_out(:,:,b,6)
         strairy_ocn(:,:,b) = a_out(:,:,b,7)
         Tref_ocn(:,:,b) = a_out(:,:,b,8)
         Qref_ocn(:,:,b) = a_out(:,:,b,9)
         alvdr_ocn(:,:,b) = a_out(:,:,b,10)
         alidr_ocn(:,:,b) = a_out(:,:,b,11)
         alvdf_ocn(:,:,b) = a_out(:,:,b,12)
         alidf_ocn(:,:,b) = a_out(:,:,b,13)
      enddo
      call ocean_mixed_layer (a_dt)
      do b = 1, nb
         a_io(:,:,b,1) = sst(:,:,b)
         a_io(:,:,b,2) = qdp(:,:,b)
         a_out(:,:,b,1) = frzmlt(:,:,b)
         a_out(:,:,b,2) = flwout_ocn(:,:,b)
         a_out(:,:,b,3) = fsens_ocn(:,:,b)
         a_out(:,:,b,4) = flat_ocn(:,:,b)
         a_out(:,:,b,5) = evap_ocn(:,:,b)
         a_out(:,:,b,6) = strairx_ocn(:,:,b)
         a_out(:,:,b,7) = strairy_ocn(:,:,b)
         a_out(:,:,b,8) = Tref_ocn(:,:,b)
         a_out(:,:,b,9) = Qref_ocn(:,:,b)
         a_out(:,:,b,10) = alvdr_ocn(:,:,b)
         a_out(:,:,b,11) = alidr_ocn(:,:,b)
         a_out(:,:,b,12) = alvdf_ocn(:,:,b)
         a_out(:,:,b,13) = alidf_ocn(:,:,b)
      enddo
      end subroutine cpcap_mixed

      ! atmo_boundary_layer('ocn') on the ocean cells of one block, as ocean_mixed_layer lists them: the four locals
      subroutine cpcap_atmo (a_tmask, a_sst, a_potT, a_uatm, a_vatm, a_wind, a_zlvl, a_Qa, a_rhoa, a_delt, a_delq, &
                 a_lhcoef, a_shcoef) bind(C, name='cpcap_atmo')
      use ice_atmo, only: atmo_boundary_layer, calc_strair
      integer(c_int) :: a_tmask(nx_block,ny_block)
      real(c_double), dimension(nx_block,ny_block) :: a_sst, a_potT, a_uatm, a_vatm, a_wind, a_zlvl, a_Qa, a_rhoa, a_delt, &
         a_delq, a_lhcoef, a_shcoef
      real(dbl_kind), dimension(nx_block,ny_block) :: sx, sy, tr, qr
      integer(int_kind) :: indxi(nx_block*ny_block), indxj(nx_block*ny_block), icells, i, j
      calc_strair = .true.
      icells = 0
      do j = 1, ny_block
      do i = 1, nx_block
         if (a_tmask(i,j) /= 0) then
            icells = icells + 1
            indxi(icells) = i
            indxj(icells) = j
         endif
      enddo
      enddo
      call atmo_boundary_layer (nx_block, ny_block, 'ocn', icells, indxi, indxj, a_sst, a_potT, a_uatm, a_vatm, a_wind, &
                                a_zlvl, a_Qa, a_rhoa, sx, sy, tr, qr, a_delt, a_delq, a_lhcoef, a_shcoef)
      end subroutine cpcap_atmo

      end module coupling_capture
